"""The SGHMC sampler on the GPU (csrc/sghmc_device.h; its users in field_kernels.hip, stencil_kernels.hip, bending_kernels.hip) against
the numpy float32 restatement of tests/_sghmc.py, bit for bit: the stateless operator with injected and with Philox noise, the fused
update of a transition against the stateless operator, everything else of a transition left alone, recovery, stream capture, the
statistics of the momentum, the refusals and the trainer.

Shapes (D,H,W).  The stateless kernel gives a thread one column (x, y) of one plane pair, 64 x 4 columns a workgroup:
  (3,3,3), (2,5,6)   one workgroup; an odd D whose last pair has no odd plane, and an even one;
  (5,6,70)           two x tiles (64 + 6), two tile rows (4 + 2), the open last pair;
  (5,9,129)          three x tiles, the last 1 wide; three tile rows, the last 1 high.
The fused updates march z segments of 64 x 4 (first order) and 32 x 8 (bending) column tiles; the shapes, and `update_seg` = 0, 2, 3,
are those of tests/test_gpu_bending.py: (7,13,70), (5,9,129), (11,13,70) with 3 chains, and one SVFFD case with cps (2,2,2).  With
`update_seg` = 3 segments start on odd planes: a thread must draw its voxel pair there too.

Every comparison is torch.equal except the Box-Muller normals themselves, which carry tests/_langevin_noise.py's tolerance."""
import copy
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

from ir_sgmcmc_amd import _lib as L
from ir_sgmcmc_amd import sghmc
from ir_sgmcmc_amd.engine import EngineConfig, TransitionEngine, irs_config
from tests import _langevin_noise as N
from tests import _sghmc as S
from tests import _transition_scalars as R
from tests.test_gpu_bending import pair24, to_dev, update_seg, white

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S3, S2, P, Bd, A, M = (3, 3, 3), (2, 5, 6), (5, 6, 70), (5, 9, 129), (7, 13, 70), (11, 13, 70)
L2, LN, ST = 'RegLoss_L2', 'RegLoss_LogNormal', 'RegLoss_Student'
GRAD, HESS = 'GradientOperator', 'HessianOperator'


def name(*parts):
    return '-'.join('x'.join(map(str, p)) if isinstance(p, tuple) else str(p) for p in parts)


def randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def sigma_field(shape, seed=2):
    return 0.5 + torch.rand(shape, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the stateless operator, injected noise: bit for bit
# ------------------------------------------------------------------------------------------------------------------------------
STATELESS = [(d, c, s) for d in (S3, S2, P, Bd) for c in (1, 3) for s in (False, True)]


@pytest.mark.parametrize('dims,Cn,with_sigma', STATELESS, ids=[name(*c) for c in STATELESS])
def test_stateless_injected_noise_bit_for_bit(dims, Cn, with_sigma):
    shape = (Cn, 3, *dims)
    v0, m0, g, eps = randn(shape, 1), randn(shape, 2), 3.0 * randn(shape, 3), randn(shape, 4)
    sigma = sigma_field(shape) if with_sigma else None
    for friction in (1.0, 0.5, 0.1):
        for T in (0.0, 0.25, 1.0):
            v, m = v0.to(DEV), m0.to(DEV)
            out = sghmc.sghmc_update(v, m, g.to(DEV), None if sigma is None else sigma.to(DEV), lr=0.4, friction=friction, temperature=T,
                                     eps=eps.to(DEV))
            assert out[0] is v and out[1] is m  # in place
            rv, rm = S.step(v0.numpy(), m0.numpy(), g.numpy(), None if sigma is None else sigma.numpy(), eps.numpy(), 0.4, friction, T)
            assert torch.equal(m.cpu(), torch.from_numpy(rm)), (friction, T)
            assert torch.equal(v.cpu(), torch.from_numpy(rv)), (friction, T)
            assert not torch.equal(v.cpu(), v0)
    # temperature 0 reads no noise at all: not the injected one either
    v, m = v0.to(DEV), m0.to(DEV)
    sghmc.sghmc_update(v, m, g.to(DEV), lr=0.4, friction=0.5, temperature=0.0, eps=torch.full(shape, float('nan'), device=DEV))
    rv, rm = S.step(v0.numpy(), m0.numpy(), g.numpy(), None, None, 0.4, 0.5, 0.0)
    assert torch.equal(v.cpu(), torch.from_numpy(rv)) and torch.equal(m.cpu(), torch.from_numpy(rm))


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the stateless operator, Philox noise: v = m = grad = 0, lr = 1/2, friction 1, T = 1 -- amp = 1 exactly, sigma a power of two:
#    m' = sigma n without a rounding, so m' / sigma is the normal itself
# ------------------------------------------------------------------------------------------------------------------------------
PHILOX = [(S3, 1, 5, 0), (S2, 3, 5, 7), (P, 3, 5, 2 ** 32 + 3), (Bd, 3, 2 ** 40 + 9, 11), (Bd, 1, 0, 2 ** 63 + 1)]


@pytest.mark.parametrize('dims,Cn,seed,iteration', PHILOX, ids=[name(*c) for c in PHILOX])
def test_stateless_philox_noise_is_the_restated_draw(dims, Cn, seed, iteration):
    shape = (Cn, 3, *dims)
    gen = torch.Generator().manual_seed(6)
    sigma = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, shape, generator=gen)]
    zero = lambda: torch.zeros(shape, device=DEV)
    v, m = zero(), zero()
    sghmc.sghmc_update(v, m, zero(), sigma.to(DEV), lr=0.5, friction=1.0, temperature=1.0, seed=seed, iteration=iteration)
    assert torch.equal(v, m)
    got = (m.cpu() / sigma).to(torch.float64).numpy()
    ref, r = S.normals(seed, iteration, Cn, dims)
    dev = np.abs(got - ref) / N.tol(r)
    print(f'sghmc/philox/{name(dims, Cn, seed, iteration)}: worst deviation / tolerance {dev.max():.4f}')
    assert dev.max() <= 1.0
    # the same counter under the forward perturbation's stream word is another draw
    other, _ = N.normals_from_words(N.noise_words(seed, iteration, Cn, dims), dims[0])
    assert np.abs(got - other).max() > 1.0
    if Cn > 1:  # chain > 0 has a draw of its own
        assert np.abs(got[1] - got[0]).max() > 1.0
    # without sigma the same normals; the call is deterministic
    v2, m2 = zero(), zero()
    sghmc.sghmc_update(v2, m2, zero(), lr=0.5, friction=1.0, temperature=1.0, seed=seed, iteration=iteration)
    assert torch.equal(m2.cpu(), m.cpu() / sigma)


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the fused update of a transition against the stateless operator (and, with injected noise, against the restatement)
# ------------------------------------------------------------------------------------------------------------------------------
def sghmc_transition(cfg, fixed, moving, v0, m0, sigma, eps, unif, options=None):
    """one transition on a fresh engine -> dict of host tensors v, m, curr_state, grad_v, plus it0 (the Philox counter before it), the
    scalars and the state after; the context is gone when this returns"""
    eng = TransitionEngine(cfg, DEV)
    try:
        eng.option('predict_variants', 0)  # every kernel variant is launched: nothing is assumed, no transition is re-run
        for k, val in (options or {}).items():
            eng.option(k, val)
        fd, md = eng.prepare(to_dev(fixed), to_dev(moving))
        if cfg.data_loss == 'GMM':
            eng.gmm_init(fd, md)
        it0 = int(eng.state().iteration)
        if cfg.sampler == 'SGHMC':
            assert tuple(eng.momentum.shape) == (cfg.no_chains, 3, *cfg.dims_v) and not bool(eng.momentum.any())
            if m0 is not None:
                eng.momentum.copy_(m0)
        else:
            assert eng.momentum is None
        v = v0.to(DEV).contiguous()
        new = lambda: torch.empty(cfg.no_chains, 3, *cfg.dims_v, device=DEV, dtype=torch.float32)
        out = {'curr_state': new(), 'grad_v': new()}
        dev = lambda t: None if t is None else t.to(DEV).contiguous()
        eng.transition(fd, md, v, dev(sigma), dev(eps), dev(unif), out)
        eng.flush()
        st = eng.state()
        return {'v': v.cpu(), 'm': None if eng.momentum is None else eng.momentum.cpu(), 'curr_state': out['curr_state'].cpu(),
                'grad_v': out['grad_v'].cpu(), 'it0': it0, 'scalars': eng.scalars(), 'state': bytes(C.string_at(C.byref(st), C.sizeof(st)))}
    finally:
        eng.__del__()


FUSED = [
    # dims, C, diff_op, family, learnable, sigma field, cps, update_seg, friction, temperature
    (A, 3, GRAD, L2, False, False, None, 0, 0.1, 1.0), (A, 3, GRAD, L2, False, True, None, 0, 0.1, 1.0),
    (A, 3, GRAD, L2, True, False, None, 2, 0.5, 1.0), (A, 3, GRAD, L2, True, True, None, 3, 0.1, 0.25),
    (A, 3, GRAD, LN, True, False, None, 3, 1.0, 1.0), (A, 3, GRAD, ST, False, True, None, 2, 0.1, 1.0),
    (Bd, 3, GRAD, L2, False, True, None, 0, 1.0, 1.0), (Bd, 3, GRAD, LN, True, True, None, 2, 0.1, 1.0),
    (Bd, 3, GRAD, ST, False, False, None, 3, 0.5, 0.0),
    (M, 3, GRAD, L2, True, False, None, 0, 0.1, 1.0), (M, 3, GRAD, L2, False, True, None, 3, 0.1, 1.0), (M, 3, GRAD, LN, True, True, None, 2, 0.5, 1.0),
    (A, 3, HESS, L2, False, False, None, 0, 0.1, 1.0), (A, 3, HESS, L2, True, True, None, 3, 0.1, 1.0),
    (A, 3, HESS, LN, True, False, None, 2, 1.0, 1.0), (A, 3, HESS, ST, False, True, None, 0, 0.5, 0.25),
    (Bd, 3, HESS, L2, False, True, None, 2, 0.1, 1.0), (Bd, 3, HESS, ST, False, False, None, 3, 0.1, 1.0),
    (M, 3, HESS, L2, True, True, None, 3, 0.5, 1.0), (M, 3, HESS, LN, True, False, None, 0, 0.1, 0.0),
    (A, 3, GRAD, L2, False, True, (2, 2, 2), 0, 0.1, 1.0), (A, 3, HESS, L2, False, True, (2, 2, 2), 3, 0.1, 1.0),
]


@pytest.mark.parametrize('dims,Cn,diff_op,reg_loss,learnable,with_sigma,cps,seg,friction,T', FUSED, ids=[name(*c) for c in FUSED])
def test_fused_update_is_the_stateless_operator(dims, Cn, diff_op, reg_loss, learnable, with_sigma, cps, seg, friction, T):
    cfg = EngineConfig(dims=dims, no_chains=Cn, cps=cps, data_loss='SSD', virtual_decimation=False, reg_loss=reg_loss, reg_learnable=learnable,
                       lr=0.05, diff_op=diff_op, seed=9, sampler='SGHMC', sghmc_friction=friction, sghmc_temperature=T)
    fixed, moving, v0, _, _ = R.make_inputs(dims, Cn, cps=cps)
    shape = (Cn, 3, *cfg.dims_v)
    v0 = v0 if tuple(v0.shape) == shape else white(shape, 21)
    m0 = 0.1 * randn(shape, 23)
    sigma = sigma_field(shape) if with_sigma else None
    dev = lambda t: None if t is None else t.to(DEV)
    with update_seg(seg):
        # Philox noise: the draw is keyed by the context's seed and the counter the transition started from
        got = sghmc_transition(cfg, fixed, moving, v0, m0, sigma, None, None)
        # injected noise: the momentum's, not the forward pass's
        eps = randn(shape, 24)
        inj = sghmc_transition(cfg, fixed, moving, v0, m0, sigma, eps, None)
    assert float(got['grad_v'].abs().max()) > 0.0 and got['it0'] == 0
    v, m = v0.to(DEV), m0.to(DEV)
    sghmc.sghmc_update(v, m, got['grad_v'].to(DEV), dev(sigma), lr=cfg.lr, friction=friction, temperature=T, seed=cfg.seed, iteration=got['it0'])
    assert torch.equal(got['m'], m.cpu())
    assert torch.equal(got['v'], v.cpu())
    assert not torch.equal(got['v'], v0) and not torch.equal(got['m'], m0)
    rv, rm = S.step(v0.numpy(), m0.numpy(), inj['grad_v'].numpy(), None if sigma is None else sigma.numpy(), eps.numpy(), cfg.lr, friction, T)
    assert torch.equal(inj['m'], torch.from_numpy(rm))
    assert torch.equal(inj['v'], torch.from_numpy(rv))
    # the forward pass saw no noise either way: the jitter is Philox in both, so everything up to the update is the same
    assert torch.equal(inj['curr_state'], got['curr_state']) and torch.equal(inj['grad_v'], got['grad_v'])
    if T > 0:
        assert not torch.equal(inj['m'], got['m'])


def test_second_transition_draws_with_the_advanced_counter():
    """two transitions: the second one's noise is keyed by iteration 1, and its momentum is the first one's"""
    dims, Cn = A, 3
    cfg = EngineConfig(dims=dims, no_chains=Cn, data_loss='SSD', virtual_decimation=False, lr=0.05, seed=4, sampler='SGHMC', sghmc_friction=0.1)
    fixed, moving, v0, _, _ = R.make_inputs(dims, Cn)
    eng = TransitionEngine(cfg, DEV)
    eng.option('predict_variants', 0)
    fd, md = eng.prepare(to_dev(fixed), to_dev(moving))
    v = v0.to(DEV).contiguous()
    grad = torch.empty_like(v)
    ref_v, ref_m = v.clone(), torch.zeros_like(v)
    for it in range(2):
        assert int(eng.state().iteration) == it
        eng.transition(fd, md, v, outputs={'grad_v': grad})
        eng.flush()
        sghmc.sghmc_update(ref_v, ref_m, grad, lr=cfg.lr, friction=0.1, temperature=1.0, seed=cfg.seed, iteration=it)
        assert torch.equal(v, ref_v) and torch.equal(eng.momentum, ref_m)


# ------------------------------------------------------------------------------------------------------------------------------
# 4. nothing else moved: against an SGLD engine that is given eps = 0
# ------------------------------------------------------------------------------------------------------------------------------
UNMOVED = [(A, 3, GRAD, 'SSD', False, None), (Bd, 3, GRAD, 'GMM', True, None), (M, 3, HESS, 'SSD', True, None), (A, 3, GRAD, 'SSD', True, (2, 2, 2))]


@pytest.mark.parametrize('dims,Cn,diff_op,data_loss,with_sigma,cps', UNMOVED, ids=[name(*c) for c in UNMOVED])
def test_nothing_else_moved(dims, Cn, diff_op, data_loss, with_sigma, cps):
    """lr = 1/16.  The reference's update is v - lr g, which the compiler contracts into one fused multiply-add; the SGHMC step
    rounds the product first.  The two agree bit for bit exactly where the product lr g is exact -- lr a power of two (tests/
    test_sghmc_host.py::test_friction_one_no_noise_no_momentum_is_the_plain_gradient_step) -- and that is where the issue's
    identity fadd(v, -x) = fsub(v, x) makes the two engines' v equal."""
    base = dict(dims=dims, no_chains=Cn, cps=cps, data_loss=data_loss, virtual_decimation=False, lr=0.0625, diff_op=diff_op, seed=3)
    fixed, moving, v0, _, unif = R.make_inputs(dims, Cn, cps=cps)
    shape = (Cn, 3, *EngineConfig(**base).dims_v)
    v0 = v0 if tuple(v0.shape) == shape else white(shape, 21)
    sigma = sigma_field(shape) if with_sigma else None
    sgld = sghmc_transition(EngineConfig(**base), fixed, moving, v0, None, sigma, torch.zeros(shape), unif)
    hmc = sghmc_transition(EngineConfig(**base, sampler='SGHMC', sghmc_friction=1.0, sghmc_temperature=0.0), fixed, moving, v0, None, sigma,
                           None, unif)
    assert torch.equal(hmc['curr_state'], sgld['curr_state']) and torch.equal(hmc['grad_v'], sgld['grad_v'])
    assert hmc['scalars'] == sgld['scalars'] and hmc['state'] == sgld['state']
    assert float(sgld['grad_v'].abs().max()) > 0.0 and not torch.equal(sgld['v'], v0)
    assert torch.equal(hmc['v'], sgld['v'])
    assert torch.equal(hmc['m'], -(0.0625 * hmc['grad_v']))  # (the product is exact)
    # with noise and momentum the forward half is still that one
    noisy = sghmc_transition(EngineConfig(**base, sampler='SGHMC', sghmc_friction=0.1), fixed, moving, v0, 0.1 * randn(shape, 5), sigma, None, unif)
    assert torch.equal(noisy['curr_state'], sgld['curr_state']) and torch.equal(noisy['grad_v'], sgld['grad_v'])
    assert noisy['scalars'] == sgld['scalars'] and noisy['state'] == sgld['state']
    assert not torch.equal(noisy['v'], sgld['v'])


# ------------------------------------------------------------------------------------------------------------------------------
# 5. / 6. recovery and stream capture
# ------------------------------------------------------------------------------------------------------------------------------
def sghmc24(seed, diff_op=GRAD):
    # (bending: w_reg well inside the stability bound of the explicit step, as in tests/test_gpu_bending.py)
    extra = dict(diff_op=HESS, w_reg=0.01) if diff_op == HESS else {}
    return TransitionEngine(EngineConfig(dims=(24, 24, 24), seed=seed, sampler='SGHMC', sghmc_friction=0.5, **extra), DEV)


@pytest.mark.parametrize('diff_op', [GRAD, HESS])
def test_misprediction_is_recovered_on_an_sghmc_chain(diff_op):
    """tests/test_gpu_bending.py::test_misprediction_is_recovered_on_a_bending_chain under SGHMC: a transition that turns out to be a
    no-op must leave v AND the momentum alone, and its re-run draws the same noise"""
    from ir_sgmcmc_amd.ops import perturb_smooth, sobolev_kernel_1d
    N_, T = 24, 6
    fixed, moving = pair24()
    v0 = perturb_smooth(randn((1, 3, N_, N_, N_), 3).to(DEV), sobolev_kernel_1d(3, 0.5))
    v0 = v0 * (9.0 / float(v0.abs().max()))
    res = {}
    for mode in (0, 3):
        eng = sghmc24(11, diff_op)
        eng.option('predict_variants', mode)
        fd, md = eng.prepare(fixed, moving)
        eng.gmm_init(fd, md)
        v = v0.clone()
        for _ in range(T):
            eng.transition(fd, md, v)
        eng.flush()
        st = eng.state()
        assert st.iteration == T
        res[mode] = (v.clone(), eng.momentum.clone(), bytes(C.string_at(C.byref(st), C.sizeof(st))), eng.scalars(), eng.recovered_transitions)
    assert res[0][4] == 0 and res[3][4] >= 1, (res[0][4], res[3][4])
    assert torch.equal(res[0][0], res[3][0]) and torch.equal(res[0][1], res[3][1]) and res[0][2] == res[3][2] and res[0][3] == res[3][3]
    assert not torch.equal(res[0][0], v0) and bool(res[0][1].any())


def test_captured_transition_matches_an_eager_one():
    N_ = 24
    fixed, moving = pair24()

    def fresh():
        eng = sghmc24(7)
        fd, md = eng.prepare(fixed, moving)
        eng.gmm_init(fd, md)
        return eng, fd, md

    eng, fd, md = fresh()
    v_plain = torch.zeros(1, 3, N_, N_, N_, device=DEV)
    for _ in range(4):
        eng.transition(fd, md, v_plain)
    eng.flush()
    sc_plain, m_plain = eng.scalars(), eng.momentum.clone()

    eng, fd, md = fresh()
    v = torch.zeros(1, 3, N_, N_, N_, device=DEV)
    eng.transition(fd, md, v)  # (lazily created resources exist before the capture)
    eng.flush()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        eng.transition(fd, md, v)
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    eng.flush()
    assert torch.equal(v, v_plain) and torch.equal(eng.momentum, m_plain) and float(v.abs().max()) > 0.0
    assert eng.scalars() == sc_plain and int(eng.state().iteration) == 4


# ------------------------------------------------------------------------------------------------------------------------------
# 7. statistics: without a gradient the momentum is an AR(1) process of known variance
# ------------------------------------------------------------------------------------------------------------------------------
def test_momentum_statistics():
    Cn, dims, a, lr, n = 2, (16, 16, 16), 0.5, 0.4, 64
    shape = (Cn, 3, *dims)
    v, m, g = (torch.zeros(shape, device=DEV) for _ in range(3))
    for it in range(n):
        sghmc.sghmc_update(v, m, g, lr=lr, friction=a, temperature=1.0, seed=13, iteration=it)
    Mn = m.numel()
    assert Mn == 24576
    _, oma, amp = S.constants(lr, a, 1.0)
    want = S.ar1_variance(amp, oma, n)
    x = m.to(torch.float64).flatten().cpu()
    var, mean = float(x.var(unbiased=False)), float(x.mean())
    margin = 5.0 * math.sqrt(2.0 / Mn)
    print(f'sghmc/statistics: variance {var:.6g} against {want:.6g} ({abs(var / want - 1.0) / margin:.3f} of the margin), mean {mean:.3g} '
          f'({abs(mean) / (5.0 * math.sqrt(want / Mn)):.3f} of the margin)')
    assert abs(var / want - 1.0) <= margin
    assert abs(mean) <= 5.0 * math.sqrt(want / Mn)
    kt = sghmc.kinetic_temperature(m, None, lr, a)
    implied = want * (1.0 - 0.5 * a) / lr  # what that variance reads as: 1 up to (1 - oma^2n)
    assert tuple(kt.shape) == (Cn,) and abs(float(kt.mean()) / implied - 1.0) <= margin + mean * mean / want
    assert implied == pytest.approx(1.0, abs=1e-6)  # (amp and oma are float32 numbers)
    # v is the running sum of the momenta
    assert bool(torch.isfinite(v).all()) and float(v.abs().max()) > 1.0


# ------------------------------------------------------------------------------------------------------------------------------
# 8. refusals
# ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_of_the_update():
    lib = L.load()
    t = torch.zeros(1, 3, 4, 4, 4, device=DEV)
    p = lambda x: C.c_void_p(x.data_ptr())
    good = dict(v=p(t), m=p(t.clone()), g=p(t.clone()), C=1, D=4, H=4, W=4, lr=0.4, a=0.5, T=1.0)

    def call(**over):
        k = {**good, **over}
        rc = lib.irs_sghmc_update(k['v'], k['m'], k['g'], None, None, k['C'], k['D'], k['H'], k['W'], k['lr'], k['a'], k['T'], 0, 0, L.stream_ptr())
        return rc, lib.irs_last_error().decode()

    assert call()[0] == 0
    for over, word in (({'v': None}, 'null'), ({'m': None}, 'null'), ({'g': None}, 'null'), ({'D': 0}, 'dims'), ({'H': 0}, 'dims'),
                       ({'W': -1}, 'dims'), ({'C': 0}, 'chains'), ({'C': L.IRS_MAX_CHAINS + 1}, 'chains'), ({'a': 0.0}, 'friction'),
                       ({'a': 1.5}, 'friction'), ({'a': float('nan')}, 'friction'), ({'T': -1.0}, 'temperature'),
                       ({'T': float('inf')}, 'temperature'), ({'lr': float('nan')}, 'lr')):
        rc, msg = call(**over)
        assert rc != 0 and 'irs_sghmc_update' in msg and word in msg, (over, msg)
    torch.cuda.synchronize()
    # the wrapper's own
    with pytest.raises(L.IrsError, match='shape of v'):
        sghmc.sghmc_update(t, t.clone()[:, :, :2], t.clone(), lr=0.4, friction=0.5)
    with pytest.raises(L.IrsError, match=r'\(C,3,D,H,W\)'):
        sghmc.sghmc_update(t[0], t[0].clone(), t[0].clone(), lr=0.4, friction=0.5)
    with pytest.raises(L.IrsError, match='GPU only'):
        sghmc.sghmc_update(t.cpu(), t.cpu(), t.cpu(), lr=0.4, friction=0.5)
    with pytest.raises(L.IrsError, match='friction'):
        sghmc.sghmc_update(t, t.clone(), t.clone(), lr=0.4, friction=0.0)


def test_refusals_of_the_setter():
    lib = L.load()
    cfg = EngineConfig(dims=(16, 16, 16), data_loss='SSD', virtual_decimation=False)
    eng = TransitionEngine(cfg, DEV)
    m = torch.zeros(1, 3, 16, 16, 16, device=DEV)
    ptr = C.c_void_p(m.data_ptr())
    for args, word in (((None, 0.5, 1.0, ptr), 'null'), ((eng._ctx, 0.5, 1.0, None), 'null'), ((eng._ctx, 0.0, 1.0, ptr), 'friction'),
                       ((eng._ctx, -0.5, 1.0, ptr), 'friction'), ((eng._ctx, 1.0001, 1.0, ptr), 'friction'),
                       ((eng._ctx, float('nan'), 1.0, ptr), 'friction'), ((eng._ctx, 0.5, -0.1, ptr), 'temperature'),
                       ((eng._ctx, 0.5, float('inf'), ptr), 'temperature'), ((eng._ctx, 0.5, float('nan'), ptr), 'temperature')):
        assert lib.irs_sghmc_set(*args) != 0
        msg = lib.irs_last_error().decode()
        assert 'irs_sghmc_set' in msg and word in msg, (args, msg)
    # after the first transition: refused, by the rule of irs_lncc_set
    f1, m1 = pair24()
    fd, md = eng.prepare({'im': f1['im'][:, :, :16, :16, :16].contiguous(), 'mask': f1['mask'][:, :, :16, :16, :16].contiguous()},
                         {'im': m1['im'][:, :, :16, :16, :16].contiguous()})
    v = torch.zeros(1, 3, 16, 16, 16, device=DEV)
    eng.transition(fd, md, v)
    eng.flush()
    assert lib.irs_sghmc_set(eng._ctx, 0.5, 1.0, ptr) != 0
    assert 'before the first transition' in lib.irs_last_error().decode()
    assert eng.momentum is None
    # before it: fine, and the edge values are accepted
    other = TransitionEngine(cfg, DEV)
    assert lib.irs_sghmc_set(other._ctx, 1.0, 0.0, ptr) == 0
    # an unknown sampler name, and z-slabs: the library and the Python owner
    with pytest.raises(ValueError, match='sampler'):
        TransitionEngine(EngineConfig(dims=(16, 16, 16), sampler='HMC'), DEV)
    from ir_sgmcmc_amd.slab import SlabEngine
    with pytest.raises(L.IrsError, match='z-slab'):
        SlabEngine(EngineConfig(dims=(16, 16, 16), sampler='SGHMC'), DEV)
    slab = SlabEngine(EngineConfig(dims=(16, 16, 16)), DEV)
    assert slab.momentum is None
    ms = torch.zeros(1, 3, slab.hi - slab.lo, 16, 16, device=DEV)
    assert lib.irs_sghmc_set(slab._ctx, 0.5, 1.0, C.c_void_p(ms.data_ptr())) != 0
    assert 'z-slab' in lib.irs_last_error().decode()


# ------------------------------------------------------------------------------------------------------------------------------
# 9. the trainer: configs/synthetic_ssd_l2_128_sghmc.json cut to 24^3 and 20 transitions
# ------------------------------------------------------------------------------------------------------------------------------
def make_trainer(tmp_path, sampler='config', **trainer_over):
    from ir_sgmcmc_amd.parse_config import ConfigParser
    from ir_sgmcmc_amd.trainer import Trainer
    cfg = json.load(open(os.path.join(ROOT, 'configs', 'synthetic_ssd_l2_128_sghmc.json')))
    cfg['trainer']['save_dir'] = str(tmp_path)
    cfg['data_loader']['args']['dims'] = [24, 24, 24]
    cfg['trainer'].update(no_iters_burn_in=4, no_samples_MCMC=16, log_period_MCMC=4, checkpoint_period=4)
    cfg['trainer']['truth']['period'] = 2
    cfg['trainer']['convergence_diagnostics']['period'] = 2
    if sampler != 'config':
        cfg['trainer'].pop('sampler')
        if sampler is not None:
            cfg['trainer']['sampler'] = sampler
    cfg['trainer'].update(trainer_over)
    config = ConfigParser.from_dict(copy.deepcopy(cfg), timestamp='t')
    dl = config.init_data_loader()
    tm, rm = config.init_transformation_and_registration_modules()
    return Trainer(config, dl, config.init_losses(), tm, rm, config.init_metrics(), device=DEV)


def digest(t):
    s = t.engine.state()
    m = t.engine.momentum
    return (t.v_curr_state.cpu(), None if m is None else m.cpu(), t.displacement_mean.cpu(), t.displacement_std.cpu(), s.iteration)


def same(a, b):
    return all(torch.equal(x, z) if isinstance(x, torch.Tensor) else x == z for x, z in zip(a, b))


def test_trainer_runs_the_sghmc_config_and_resumes_bit_for_bit(tmp_path):
    a = make_trainer(tmp_path / 'a')
    ec = a._engine_config()
    assert (ec.sampler, ec.sghmc_friction, ec.sghmc_temperature) == ('SGHMC', 0.1, 1.0)
    torch.manual_seed(0)
    a.run()
    a.engine.flush()
    assert bool(torch.isfinite(a.v_curr_state).all()) and float(a.v_curr_state.abs().max()) > 0.0 and bool(a.engine.momentum.any())
    res = a.metrics.result()
    kt = [res[f'MCMC/chain_{i}/sampler/kinetic_temperature'] for i in range(2)]
    assert all(math.isfinite(x) and x > 0.0 for x in kt)
    assert a.sampler_summary['options'] == {'type': 'SGHMC', 'friction': 0.1, 'temperature': 1.0}
    # the last value logged is that of the momentum at the last sample (the speed test behind the chain runs transitions of its own)
    end = torch.load(a.config.save_dirs['checkpoints'] / 'checkpoint_0000020.pt', map_location='cpu', weights_only=True)
    # (a float64 mean of 82944 squares, summed in another order on the host than on the device: 1e-12 is a thousand times that)
    assert a.sampler_summary['kinetic_temperature'] == pytest.approx(sghmc.kinetic_temperature(end['momentum'], None, ec.lr, 0.1).tolist(),
                                                                      rel=1e-12)
    assert 'momentum' in a.state_dict() and torch.equal(a.state_dict()['momentum'], a.engine.momentum.cpu())
    ck = a.config.save_dirs['checkpoints'] / 'checkpoint_0000004.pt'
    assert ck.is_file()
    b = make_trainer(tmp_path / 'b', resume=str(ck))
    torch.manual_seed(0)
    b.run()
    assert same(digest(a), digest(b))
    # a checkpoint without the momentum, taken after transitions have run, is refused
    sd = torch.load(ck, map_location='cpu', weights_only=True)
    assert 'momentum' in sd and int(sd['sample_no']) == 4
    del sd['momentum']
    stripped = tmp_path / 'stripped.pt'
    torch.save(sd, stripped)
    c = make_trainer(tmp_path / 'c', resume=str(stripped))
    with pytest.raises(ValueError, match='holds no momentum'):
        c.run()


def test_trainer_without_the_option_is_the_trainer_as_it_is(tmp_path):
    runs = {}
    for key, sampler in (('absent', None), ('sgld', {'type': 'SGLD'})):
        t = make_trainer(tmp_path / key, sampler=sampler)
        assert t.sampler_options is None and t._engine_config().sampler == 'SGLD'
        torch.manual_seed(0)
        t.run()
        t.engine.flush()
        assert t.engine.momentum is None and t.sampler_summary is None and 'momentum' not in t.state_dict()
        assert not [k for k in t.metrics.result() if 'sampler' in k]
        runs[key] = digest(t)
    assert same(runs['absent'], runs['sgld'])
    # the reference's scheme, driven by hand from the same start: 20 transitions of an engine of that config on the trainer's pair
    eng = TransitionEngine(t._engine_config(), DEV)
    fd, md = eng.prepare(t._fixed, t._moving)
    t._set_hyper_parameters(eng)
    v = torch.zeros_like(t.v_curr_state)
    for _ in range(20):
        eng.transition(fd, md, v)
    eng.flush()
    end = torch.load(t.config.save_dirs['checkpoints'] / 'checkpoint_0000020.pt', map_location='cpu', weights_only=True)
    assert torch.equal(v.cpu(), end['v_curr_state']) and int(eng.state().iteration) == 20 and 'momentum' not in end
