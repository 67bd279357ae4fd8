"""The three pieces of hand-written HIP that close a transition, each against a float64 restatement of that piece ALONE
(tests/_transition_scalars.py) fed the arrays the GPU itself wrote: the mixture statistics with the GMM Adam step (residual `z` in;
n, alpha, the raw gradients through the Adam moments, the stepped parameters and the data term out), the regulariser scalars
(evaluated at the GPU's own energy) and the update stencil element by element (moving image identically zero: grad_v is the
regulariser half alone).  No oracle transition runs here, so the cell-boundary flips of the warp and of the squaring steps do not
enter and the tolerances are rounding-level; tests/test_transition_scalars_host.py proves that they see the mistakes they are for.

Shapes: the smallest that exercise the launch geometry (statistics tile 64 x 8, update / energy tiles 64 x 4 with a one-voxel halo,
a ring of 4 planes, segments of at least 4 planes): (7,13,70) a full and a 6-wide x tile, ragged tile rows, segments 4 + 3;
(5,9,129) three x tiles, the last 1 voxel wide, a 1-row last tile row, a 1-plane last segment; (12,8,64) exact multiples (the halo
column and row lie outside the volume); (11,13,70) for several chains (segments 4 + 4 + 3)."""
import math

import pytest
import torch

from ir_sgmcmc_amd.engine import EngineConfig, TransitionEngine
from tests import _transition_scalars as R
from tests._report import check

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F64 = torch.float64
A, B, E, M = (7, 13, 70), (5, 9, 129), (12, 8, 64), (11, 13, 70)


def to_dev(d):
    return {k: v.to(DEV).contiguous() for k, v in d.items()}


def outputs_for(cfg):
    C, dv, d = cfg.no_chains, cfg.dims_v, cfg.dims
    z = lambda *s: torch.empty(*s, device=DEV, dtype=torch.float32)
    return {'curr_state': z(C, 3, *dv), 'residuals': z(C, 1, *d), 'grad_v': z(C, 3, *dv)}


def check_each(test, key, a, b, tol):
    """|a - b| <= tol element by element; the parity report gets the worst deviation in units of its tolerance"""
    a, b, tol = (torch.as_tensor(x, dtype=F64).cpu() for x in (a, b, tol))
    exact = (a == b) | (a.isnan() & b.isnan())
    return check(test, key + ' [deviation / tolerance]', torch.where(exact, torch.zeros_like(tol), (a - b).abs() / tol), torch.zeros_like(tol), 1.0)


def make_mask(kind, base, C):
    """(1 or C,1,D,H,W) bool"""
    D, H, W = base.shape[-3:]
    zz, yy, xx = torch.meshgrid(torch.arange(D), torch.arange(H), torch.arange(W), indexing='ij')
    if kind == 'synthetic':
        m = base[0, 0]
    elif kind == 'checkerboard':        # every lag pair has a member off the mask: the three covariances are exactly 0
        m = (xx + yy + zz) % 2 == 0
    elif kind == 'seam_planes':         # the only D-lag pairs straddle the seam between the first two 4-plane segments
        m = (zz == 3) | (zz == 4)
    elif kind == 'faces':               # voxels whose lag partners lie outside the volume, and on the low x face
        m = base[0, 0] | (xx == 0) | (xx == W - 1) | (yy == H - 1) | (zz == D - 1)
    elif kind == 'per_chain':           # chain c's mask rolled by c voxels along W
        return torch.stack([base[0].roll(c, dims=-1) for c in range(C)]).contiguous()
    return m.view(1, 1, D, H, W).contiguous()


def engine(cfg, options):
    eng = TransitionEngine(cfg, DEV)
    eng.option('predict_variants', 0)   # every kernel variant is launched: nothing is assumed, no transition is re-run
    for k, v in options.items():
        eng.option(k, v)
    return eng


# ------------------------------------------------------------------------------------------------------------------------------
# a. mixture statistics and GMM step
# ------------------------------------------------------------------------------------------------------------------------------
MIXTURE_CASES = [
    # dims, C, K, mask, config, options, Adam step count before
    (A, 1, 4, 'synthetic', {}, {}, 0), (B, 1, 4, 'synthetic', {}, {}, 0), (E, 1, 4, 'synthetic', {}, {}, 0),
    (A, 1, 5, 'synthetic', {}, {}, 0), (B, 1, 5, 'synthetic', {}, {}, 0), (E, 1, 5, 'synthetic', {}, {}, 0),
    (A, 1, 1, 'synthetic', {}, {}, 0), (A, 1, 2, 'synthetic', {}, {}, 0), (A, 1, 8, 'synthetic', {}, {}, 0),
    (A, 1, 4, 'checkerboard', {}, {}, 0), (B, 1, 5, 'checkerboard', {}, {}, 0),
    (E, 1, 4, 'faces', {}, {}, 0), (B, 1, 8, 'faces', {}, {}, 0), (A, 1, 2, 'faces', {}, {}, 0),
    (M, 1, 4, 'seam_planes', {}, {}, 0), (M, 1, 5, 'seam_planes', {}, {}, 0),
    (A, 1, 4, 'synthetic', {}, {}, 25), (B, 1, 8, 'synthetic', {}, {}, 25),
    (A, 1, 4, 'synthetic', {'virtual_decimation': False}, {}, 0), (B, 1, 5, 'synthetic', {'virtual_decimation': False}, {}, 0),
    (M, 3, 4, 'per_chain', {}, {'data_batch': 1}, 0), (M, 3, 4, 'per_chain', {}, {'data_batch': 0}, 0),
    (M, 3, 5, 'per_chain', {}, {'data_batch': 1}, 0), (M, 3, 5, 'per_chain', {}, {'data_batch': 0}, 0),
    (A, 2, 1, 'synthetic', {'data_loss': 'SSD'}, {}, 0), (B, 2, 1, 'faces', {'data_loss': 'SSD'}, {}, 0),
]


def case_id(c):
    return '-'.join(['x'.join(map(str, c[0]))] + [str(x) if not isinstance(x, dict) else ','.join(f'{k}={v}' for k, v in x.items()) for x in c[1:]]).replace('--', '-')


@pytest.mark.parametrize('dims,C,K,mask_kind,kw,options,step0', MIXTURE_CASES, ids=[case_id(c) for c in MIXTURE_CASES])
def test_mixture_statistics_and_gmm_step(dims, C, K, mask_kind, kw, options, step0):
    cfg = EngineConfig(dims=dims, no_chains=C, gmm_components=K, lr=0.05, **kw)
    h = R.hyper_from_engine(cfg)
    gmm = cfg.data_loss == 'GMM'
    fixed, moving, v0, eps, unif = R.make_inputs(dims, C)
    fixed = {'im': fixed['im'], 'mask': make_mask(mask_kind, fixed['mask'], C)}
    eng = engine(cfg, options)
    fd, md = eng.prepare(to_dev(fixed), to_dev(moving))
    eng.gmm_init(fd, md)
    st = eng.state()
    if gmm:     # the hand-set mixture (well away from its optimum: tests/test_transition_scalars_host.py), known moments
        ls, lg = R.hand_set_mixture(fixed, moving, K)
        for k in range(K):
            st.gmm_log_std[k], st.gmm_logits[k] = float(ls[k]), float(lg[k])
            for i in range(2):
                st.gmm_adam_m[i][k] = 0.0 if step0 == 0 else (30.0 - 17.0 * k) * (1 + i)
                st.gmm_adam_v[i][k] = 0.0 if step0 == 0 else 400.0 + 90.0 * k + 50.0 * i
        st.gmm_adam_step[0] = st.gmm_adam_step[1] = step0
        eng.set_state(st)
        st = eng.state()
    state0 = {'log_std': torch.tensor(list(st.gmm_log_std)[:K], dtype=F64), 'logits': torch.tensor(list(st.gmm_logits)[:K], dtype=F64),
              'm': torch.tensor([list(r)[:K] for r in st.gmm_adam_m], dtype=F64), 'v': torch.tensor([list(r)[:K] for r in st.gmm_adam_v], dtype=F64),
              'step': list(st.gmm_adam_step)}
    v = v0.to(DEV).contiguous()
    out = outputs_for(cfg)
    eng.transition(fd, md, v, None, eps.to(DEV), unif.to(DEV), out)
    sc, st = eng.scalars(), eng.state()
    z = out['residuals'].cpu()
    assert bool(torch.isfinite(z).all())

    recs, final = R.mixture_stage_with_spread(z, fixed['mask'], state0, h)
    T = 'stage/mixture/' + case_id((dims, C, K, mask_kind, kw, options, step0))
    for c, r in enumerate(recs):
        assert sc['n_mask'][c] == r['n'], (c, sc['n_mask'][c], r['n'])
        assert math.isfinite(r['alpha'])
        if mask_kind == 'checkerboard' or not cfg.virtual_decimation:
            assert r['alpha'] == 1.0 and sc['alpha'][c] == 1.0, (sc['alpha'][c], r['alpha'], r['corr'])
        else:
            assert 0.0 < r['alpha'] <= 1.0  # (K = 2 sits at the cap on every axis, K = 1 along D; K >= 4 on none: all three lag sums matter)
            check_each(T, 'alpha', sc['alpha'][c], r['alpha'], R.tol_alpha(r['corr']) * r['alpha'])
        # the data term: the GPU's alpha x sum of -log p with the parameters this chain's step left.  One chain: the parameters
        # read back from the GPU, 1e-5 relative.  Several: the serial recursion's, with the spread that their tolerance allows.
        if C == 1 and gmm:
            par = (torch.tensor(list(st.gmm_log_std)[:K], dtype=F64), torch.tensor(list(st.gmm_logits)[:K], dtype=F64))
        else:
            par = (r['log_std'], r['logits'])
        nll = float((R.mixture_eval(z[c, 0], par[0], par[1], h)[0] * fixed['mask'][c if fixed['mask'].shape[0] > 1 else 0, 0].to(F64)).sum())
        ref = sc['alpha'][c] * nll
        check_each(T, 'data_term', sc['data_term'][c], ref, 1e-5 * abs(ref) + (0.0 if C == 1 else r['tol_data']))
    if not gmm:
        return
    last = recs[-1]
    assert list(st.gmm_adam_step) == [step0 + C, step0 + C]
    m = torch.tensor([list(r)[:K] for r in st.gmm_adam_m], dtype=F64)
    vv = torch.tensor([list(r)[:K] for r in st.gmm_adam_v], dtype=F64)
    if C == 1:     # the raw gradient: m = beta1 m0 + (1 - beta1) g
        g_gpu = (m - h.beta1 * state0['m']) / (1.0 - h.beta1)
        check_each(T, 'gradient log_std (from adam m)', g_gpu[0], last['g'][0], last['tol_g'][0])
        check_each(T, 'gradient logits (from adam m)', g_gpu[1], last['g'][1], last['tol_g'][1])
    else:
        check_each(T, 'adam m (log_std, logits)', m, final['m'], last['tol_m'])
    check_each(T, 'adam v (log_std, logits)', vv, final['v'], last['tol_v'])
    check_each(T, 'gmm_log_std', list(st.gmm_log_std)[:K], last['log_std'], last['tol_param'][0])
    check_each(T, 'gmm_logits', list(st.gmm_logits)[:K], last['logits'], last['tol_param'][1])


# ------------------------------------------------------------------------------------------------------------------------------
# b. regulariser scalars and c. the update stencil: moving image identically zero, SSD, no virtual decimation
# ------------------------------------------------------------------------------------------------------------------------------
L2, LN, ST, LNL2 = 'RegLoss_L2', 'RegLoss_LogNormal', 'RegLoss_Student', 'RegLoss_LogNormal_L2'
REG_CASES = [
    # dims, C, family, learnable, sigma field, energy_in_update (None: default), cps
    (A, 1, L2, False, False, None, None), (A, 3, L2, False, True, None, None), (A, 1, L2, True, True, None, None), (A, 3, L2, True, False, None, None),
    (A, 1, LN, False, False, None, None), (A, 3, LN, False, True, None, None), (A, 1, LN, True, True, None, None), (A, 3, LN, True, False, None, None),
    (A, 1, ST, False, True, None, None), (A, 3, ST, False, False, None, None), (A, 1, LNL2, False, False, None, None), (A, 3, LNL2, False, True, None, None),
    (A, 2, L2, False, True, 0, None), (A, 2, L2, True, False, 0, None), (A, 2, L2, True, True, 1, None), (A, 2, LNL2, False, True, 0, None),
    (A, 2, LN, True, True, None, None), (A, 2, ST, False, True, None, None),
    (B, 2, L2, False, True, 1, None), (B, 2, L2, True, True, 0, None), (B, 1, LN, True, True, None, None), (B, 1, ST, False, False, None, None),
    (E, 2, L2, True, True, 1, None), (E, 2, L2, False, True, 0, None), (E, 1, LN, True, False, None, None), (E, 1, LNL2, False, True, 1, None),
    (A, 1, L2, True, True, 1, (3, 3, 3)), (A, 2, L2, False, False, 0, (3, 3, 3)), (A, 1, LN, True, True, None, (3, 3, 3)), (B, 2, ST, False, True, None, (3, 3, 3)),
]


@pytest.mark.parametrize('dims,C,reg_loss,learnable,sigma_field,eiu,cps', REG_CASES, ids=[case_id(c) for c in REG_CASES])
def test_regulariser_scalars_and_update_stencil(dims, C, reg_loss, learnable, sigma_field, eiu, cps):
    cfg = EngineConfig(dims=dims, no_chains=C, cps=cps, data_loss='SSD', virtual_decimation=False, reg_loss=reg_loss, reg_learnable=learnable, lr=0.05)
    h = R.hyper_from_engine(cfg)
    fixed, moving, v0, eps, unif = R.make_inputs(dims, C, cps=cps)
    moving = {'im': torch.zeros_like(moving['im'])}
    # a preconditioner FIELD drawn per element and per channel from U(0.5, 1.5): the three channels and every plane differ
    sigma = 0.5 + torch.rand(v0.shape, generator=torch.Generator().manual_seed(2)) if sigma_field else None
    eng = engine(cfg, {} if eiu is None else {'energy_in_update': eiu})
    fd, md = eng.prepare(to_dev(fixed), to_dev(moving))
    st0 = eng.state()
    assert list(st0.reg_adam_m) == [0.0, 0.0] and list(st0.reg_adam_v) == [0.0, 0.0] and list(st0.reg_adam_step) == [0, 0]
    par0 = list(st0.reg_param)
    v = v0.to(DEV).contiguous()
    out = outputs_for(cfg)
    eng.transition(fd, md, v, None if sigma is None else sigma.to(DEV), eps.to(DEV), unif.to(DEV), out)
    sc, st = eng.scalars(), eng.state()
    v_s, grad = out['curr_state'].cpu(), out['grad_v'].cpu()
    T = 'stage/regulariser/' + case_id((dims, C, reg_loss, learnable, sigma_field, eiu, cps))

    # b. the energy of the GPU's own v_s; then everything else AT the GPU's energy: fp64 scalar arithmetic on the same numbers
    y_gpu = torch.tensor(sc['reg_energy'], dtype=F64)
    y = R.reg_energy(v_s)
    check_each(T, 'reg_energy', y_gpu, y, 1e-6 * y)
    s = R.reg_scalars(y_gpu, par0, h)
    check_each(T, 'reg_term', sc['reg_term'], s['reg_term'], 1e-10 * s['reg_term_scale'])
    n = len(s['grads'])
    assert n == (0 if not learnable else 2 if reg_loss == LN else 1)
    assert list(st.reg_adam_step)[:n] == [1] * n
    if n:
        g, gs = torch.tensor(s['grads'], dtype=F64), torch.tensor(s['grads_scale'], dtype=F64)
        tol_g = 1e-10 * gs
        check_each(T, 'gradient reg_param (from adam m)', torch.tensor(list(st.reg_adam_m)[:n], dtype=F64) / (1.0 - h.beta1), g, tol_g)
        check_each(T, 'adam v reg_param', list(st.reg_adam_v)[:n], (1.0 - h.beta2) * g * g, (1.0 - h.beta2) * (2.0 * g.abs() * tol_g + tol_g ** 2))
        p = torch.tensor(R.reg_step(s, par0, [0.0] * n, [0.0] * n, [0] * n, h)[0], dtype=F64)
        spread = torch.zeros(n, dtype=F64)
        for sign in (-1.0, 1.0):
            moved = dict(s, grads=[float(x) for x in g + sign * tol_g])
            spread = torch.maximum(spread, (torch.tensor(R.reg_step(moved, par0, [0.0] * n, [0.0] * n, [0] * n, h)[0], dtype=F64) - p).abs())
        p0 = torch.tensor(par0[:n], dtype=F64)
        check_each(T, 'reg_param', list(st.reg_param)[:n], p, spread + 1e-10 * (p0.abs() + (p - p0).abs()))
    else:
        assert list(st.reg_param) == par0 and list(st.reg_adam_m) == [0.0, 0.0]

    # c. grad_v = sigma^2 2 coef D^T D v_s, element by element: the data part is a sum of products with image values that are
    # all 0, and zeros survive the adjoint squaring steps (and the FFD adjoint)
    assert float(v_s.abs().max()) > 0.5
    ref = R.reg_grad_v(v_s, s['coef'], sigma)
    check_each(T, 'grad_v', grad, ref, R.tol_grad_v(ref, s['coef'], v_s, sigma))
    check_each(T, 'v_new', v.cpu(), v0.to(F64) - h.lr * grad.to(F64), R.tol_v_new(v0, h.lr, grad))
