"""The bending-energy prior on the GPU (csrc/bending_kernels.hip) against the float64 closed form of tests/_bending.py: the energy,
the gradient element by element, the update stencil inside a transition for every regulariser family, exact integer cases bit for
bit, the data half of grad_v left alone, recovery and stream capture, the autograd layer, the refusals and the trainer.

Geometry of the three kernels: a workgroup owns a 32 x 8 column tile of one component with a two-voxel halo (36 x 12 staged), an LDS
ring of 8 planes, and marches a z segment with a run-in of two planes on either side; segments of the gradient / update are at
least 4 planes long by size (`update_seg` forces a length), those of the energy at least 8.  The shapes (D,H,W), in those terms:
  (3,3,3), (2,5,6)  the smallest legal volumes: one tile, the halo clamps on every side, (2,5,6) has no pure term along z;
  (7,13,70)   two full x tiles and a 6-wide one, a full tile row and a 5-row one, segments 4 + 3 whose two-plane run-ins overlap;
  (5,9,129)   four full x tiles and one 1 voxel wide, whose low halo spans two columns of the neighbour tile and whose high halo
              clamps; a 1-row last tile row; segments 4 + 1;
  (12,8,64)   exact multiples of the tile and of the segment: every halo beyond the last tile lies outside the volume;
  (11,13,70)  three chains, segments 4 + 4 + 3.
`update_seg` = 2 and 3 make segments shorter than the ring (and than the run-in of both sides together).

The rounding bound.  One output of bending_grad_march_kernel is fed by K = 66 float32 roundings (products with the weights 0, 1, 2
are exact): per axis three second differences of 2 roundings and 2 to combine them = 8, three axes = 24; per axis pair three
first-order lines of 3 and 3 across them = 12, three pairs = 36; the two sums of three terms 2 + 2; pure + 2 mixed 1; the product
with 2 scale_c 1.  Every rounding is relative to a partial sum whose magnitude is at most 2 |H|^T W |H| |v| = grad_abs(v), so
|g_hip - g_64| <= K 2^-24 grad_abs(v) (fused multiply-adds only remove roundings).  A coefficient wrong by 1 in any tap errs by
|v|, hundreds of times that.  In a transition the product with 2 coef, the float32 cast of 2 coef, sigma^2 and its product add 4."""
import contextlib
import copy
import ctypes as C
import gc
import json
import os

import pytest
import torch

from ir_sgmcmc_amd import _lib as L
from ir_sgmcmc_amd import bending
from ir_sgmcmc_amd.engine import EngineConfig, TransitionEngine, irs_config
from tests import _bending as B
from tests import _transition_scalars as R
from tests._report import check

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 66
U = 2.0 ** -24
S3, S2, A, Bd, E, M = (3, 3, 3), (2, 5, 6), (7, 13, 70), (5, 9, 129), (12, 8, 64), (11, 13, 70)
FIELDS = [(S3, 1), (S2, 1), (A, 1), (Bd, 1), (E, 1), (M, 3)]


def white(shape, seed):
    """white noise, uniform in [-1, 1]: no cancellation in the stencil, so the a-priori bound is the size of the result"""
    return (2.0 * torch.rand(shape, generator=torch.Generator().manual_seed(seed)) - 1.0).contiguous()


def field(dims, Cn, seed=5):
    return white((Cn, 3, *dims), seed)


def name(dims, *rest):
    return '-'.join(['x'.join(map(str, dims))] + [str(r) for r in rest])


def check_each(test, key, a, b, tol):
    """|a - b| <= tol element by element; the parity report gets the worst deviation in units of its tolerance"""
    a, b, tol = (torch.as_tensor(x, dtype=F64).cpu() for x in (a, b, tol))
    exact = (a == b) | (a.isnan() & b.isnan())
    dev = torch.where(exact, torch.zeros_like(a), (a - b).abs() / tol)
    print(f'{test}: {key}: worst deviation / tolerance {float(dev.max()):.4f}')
    return check(test, key + ' [deviation / tolerance]', dev, torch.zeros_like(dev), 1.0)


@contextlib.contextmanager
def update_seg(n):
    """the process-wide segment length of the update kernels; it may only change while no context is alive"""
    gc.collect()
    if n:
        L.option_set('update_seg', n)
    try:
        yield
    finally:
        gc.collect()
        if n:
            L.option_set('update_seg', 0)


# ------------------------------------------------------------------------------------------------------------------------------
# the two stateless operators
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dims,Cn', FIELDS, ids=[name(*f) for f in FIELDS])
def test_energy(dims, Cn):
    v = field(dims, Cn)
    y = bending.bending_energy(v.to(DEV))
    again = bending.bending_energy(v.to(DEV))
    ref = B.energy(v)
    assert y.dtype == F64 and tuple(y.shape) == (Cn,) and bool((ref > 0).all())
    check_each('bending/energy/' + name(dims, Cn), 'y', y, ref, 1e-5 * ref)
    assert torch.equal(y, again)  # fixed summation order, no atomics


GRAD_CASES = [(d, c, 0) for d, c in FIELDS] + [(d, c, s) for s in (2, 3) for d, c in ((S2, 1), (A, 1), (Bd, 1), (M, 3))]


@pytest.mark.parametrize('dims,Cn,seg', GRAD_CASES, ids=[name(*c) for c in GRAD_CASES])
def test_gradient_per_element(dims, Cn, seg):
    v = field(dims, Cn)
    scale = torch.tensor([0.75, -3.0, 1.0 / 3.0][:Cn])
    with update_seg(seg):
        g = bending.bending_energy_grad(v.to(DEV)).cpu()
        gs = bending.bending_energy_grad(v.to(DEV), scale.to(DEV)).cpu()
    ref, mag = B.grad(v), B.grad_abs(v)
    assert float(ref.abs().max()) > 10.0
    T = 'bending/gradient/' + name(dims, Cn, seg)
    check_each(T, 'dy/dv', g, ref, K * U * mag)
    s = scale.to(F64).view(-1, 1, 1, 1, 1)
    check_each(T, 'scale dy/dv', gs, s * ref, K * U * s.abs() * mag)


def test_gradient_wrapper_checks():
    v = field(A, 2).to(DEV)
    assert torch.equal(bending.bending_energy_grad(v, 2.0), bending.bending_energy_grad(v, torch.tensor([2.0, 2.0])))
    with pytest.raises(L.IrsError, match='one value per chain'):
        bending.bending_energy_grad(v, torch.ones(3))
    with pytest.raises(L.IrsError, match=r'\(C,3,D,H,W\)'):
        bending.bending_energy(v[:, :2])
    with pytest.raises(L.IrsError, match='float32'):
        bending.bending_energy(v.double())
    with pytest.raises(L.IrsError, match='GPU only'):
        bending.bending_energy(v.cpu())


# ------------------------------------------------------------------------------------------------------------------------------
# the update stencil in a transition: moving image identically zero, so grad_v is the regulariser half alone
# ------------------------------------------------------------------------------------------------------------------------------
def to_dev(d):
    return {k: v.to(DEV).contiguous() for k, v in d.items()}


def one_transition(cfg, fixed, moving, v0, sigma, eps, unif, options=None):
    """one transition on a fresh engine -> (v after, curr_state, grad_v, scalars, reg_param before), all on the host; the context is
    gone when this returns"""
    eng = TransitionEngine(cfg, DEV)
    try:
        eng.option('predict_variants', 0)  # every kernel variant is launched: nothing is assumed, no transition is re-run
        for k, val in (options or {}).items():
            eng.option(k, val)
        fd, md = eng.prepare(to_dev(fixed), to_dev(moving))
        if cfg.data_loss == 'GMM':
            eng.gmm_init(fd, md)
        st0 = eng.state()
        par0 = list(st0.reg_param)
        v = v0.to(DEV).contiguous()
        new = lambda: torch.empty(cfg.no_chains, 3, *cfg.dims_v, device=DEV, dtype=torch.float32)
        out = {'curr_state': new(), 'grad_v': new()}
        dev = lambda t: None if t is None else t.to(DEV).contiguous()
        eng.transition(fd, md, v, dev(sigma), dev(eps), dev(unif), out)
        sc = eng.scalars()
        return v.cpu(), out['curr_state'].cpu(), out['grad_v'].cpu(), sc, par0
    finally:
        eng.__del__()


L2, LN, ST = 'RegLoss_L2', 'RegLoss_LogNormal', 'RegLoss_Student'
UPDATE_CASES = [
    # dims, C, family, learnable, sigma field, cps, update_seg
    (A, 1, L2, False, False, None, 0), (A, 1, L2, False, True, None, 0), (A, 1, L2, True, False, None, 0), (A, 1, L2, True, True, None, 0),
    (A, 1, LN, True, False, None, 0), (A, 1, LN, True, True, None, 0), (A, 1, ST, False, False, None, 0), (A, 1, ST, False, True, None, 0),
    (S3, 1, L2, False, True, None, 0), (S2, 1, LN, True, False, None, 0),
    (Bd, 1, L2, True, True, None, 0), (Bd, 1, ST, False, False, None, 0), (E, 1, LN, True, True, None, 0), (E, 1, L2, False, False, None, 0),
    (M, 3, L2, False, True, None, 0), (M, 3, LN, True, False, None, 0), (M, 3, ST, False, True, None, 0),
    (A, 1, L2, False, True, (2, 2, 2), 0),
    (A, 1, L2, False, True, None, 2), (A, 1, LN, True, False, None, 3), (Bd, 1, ST, False, True, None, 2), (M, 3, L2, True, True, None, 3),
]


@pytest.mark.parametrize('dims,Cn,reg_loss,learnable,sigma_field,cps,seg', UPDATE_CASES, ids=[name(*c) for c in UPDATE_CASES])
def test_update_stencil_in_a_transition(dims, Cn, reg_loss, learnable, sigma_field, cps, seg):
    cfg = EngineConfig(dims=dims, no_chains=Cn, cps=cps, data_loss='SSD', virtual_decimation=False, reg_loss=reg_loss,
                       reg_learnable=learnable, lr=0.05, diff_op='HessianOperator')
    h = R.hyper_from_engine(cfg)
    fixed, moving, _, _, unif = R.make_inputs(dims, Cn, cps=cps)
    moving = {'im': torch.zeros_like(moving['im'])}
    v0 = white((Cn, 3, *cfg.dims_v), 21)
    eps = torch.randn(v0.shape, generator=torch.Generator().manual_seed(22))
    sigma = 0.5 + torch.rand(v0.shape, generator=torch.Generator().manual_seed(2)) if sigma_field else None
    with update_seg(seg):
        v, v_s, grad, sc, par0 = one_transition(cfg, fixed, moving, v0, sigma, eps, unif)
    T = 'bending/update/' + name(dims, Cn, reg_loss, learnable, sigma_field, cps, seg)

    y = B.energy(v_s)
    check_each(T, 'reg_energy', sc['reg_energy'], y, 1e-5 * y)
    term = R.reg_scalars(y, par0, h)['reg_term']
    check_each(T, 'reg_term', sc['reg_term'], term, 1e-5 * term.abs())

    # grad_v = sigma^2 2 coef H^T W H v_s, the coefficient evaluated in float64 at the GPU's own energy
    coef = R.reg_scalars(torch.tensor(sc['reg_energy'], dtype=F64), par0, h)['coef'].view(-1, 1, 1, 1, 1)
    s2 = 1.0 if sigma is None else sigma.to(F64) ** 2
    assert float(v_s.abs().max()) > 0.1
    check_each(T, 'grad_v', grad, s2 * coef * B.grad(v_s), (K + 4) * U * s2 * coef.abs() * B.grad_abs(v_s))
    check_each(T, 'v_new', v, v0.to(F64) - h.lr * grad.to(F64), R.tol_v_new(v0, h.lr, grad))
    assert not torch.equal(v, v0)


# ------------------------------------------------------------------------------------------------------------------------------
# bit for bit: integer fields, w_reg = 2 (2 coef = 2), lr = 1/4, sigma from {1/2, 1, 2}: every operation is exact in float32 in
# any order (|H^T W H v| <= 144 x 8, times 2 x 4: far below 2^24)
# ------------------------------------------------------------------------------------------------------------------------------
EXACT_CASES = [(A, False, 0), (A, True, 0), (Bd, False, 0), (Bd, True, 0), (A, True, 3), (Bd, True, 2)]


@pytest.mark.parametrize('dims,sigma_field,seg', EXACT_CASES, ids=[name(*c) for c in EXACT_CASES])
def test_exact_cases_bit_for_bit(dims, sigma_field, seg):
    Cn = 2
    cfg = EngineConfig(dims=dims, no_chains=Cn, sobolev_s=0, uniform_noise=0.0, data_loss='SSD', virtual_decimation=False, reg_loss=L2,
                       w_reg=2.0, lr=0.25, diff_op='HessianOperator')
    fixed, moving, _, _, _ = R.make_inputs(dims, Cn)
    moving = {'im': torch.zeros_like(moving['im'])}
    gen = torch.Generator().manual_seed(31)
    v0 = torch.randint(-8, 9, (Cn, 3, *dims), generator=gen).to(torch.float32)
    sigma = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, v0.shape, generator=gen)] if sigma_field else None
    with update_seg(seg):
        v, v_s, grad, sc, _ = one_transition(cfg, fixed, moving, v0, sigma, torch.zeros_like(v0), None)
    assert torch.equal(v_s, v0)
    s2 = 1.0 if sigma is None else sigma.to(F64) ** 2
    ref = s2 * B.grad(v0)  # coef = w / 2 = 1
    assert float(ref.abs().max()) < 2.0 ** 20 and float(ref.abs().max()) > 100.0
    assert torch.equal(grad.to(F64), ref)
    assert torch.equal(v.to(F64), v0.to(F64) - 0.25 * ref)
    assert sc['reg_energy'] == [float(x) for x in B.energy(v0)]  # integers below 2^24 squared and summed in double: exact as well


# ------------------------------------------------------------------------------------------------------------------------------
# the data half of grad_v is what it was: a bending engine and a first-order engine on a real pair differ by the regulariser alone
# ------------------------------------------------------------------------------------------------------------------------------
def test_data_half_untouched():
    dims, Cn = A, 2
    fixed, moving, v0, eps, unif = R.make_inputs(dims, Cn)
    res = {}
    for op in ('HessianOperator', 'GradientOperator'):
        cfg = EngineConfig(dims=dims, no_chains=Cn, data_loss='SSD', virtual_decimation=False, reg_loss=L2, lr=0.05, diff_op=op)
        res[op] = one_transition(cfg, fixed, moving, v0, None, eps, unif)
    h = R.hyper_from_engine(cfg)
    (_, vs_b, g_b, sc_b, par0), (_, vs_1, g_1, sc_1, _) = res['HessianOperator'], res['GradientOperator']
    assert torch.equal(vs_b, vs_1)
    coef = R.reg_scalars(torch.tensor(sc_b['reg_energy'], dtype=F64), par0, h)['coef'].view(-1, 1, 1, 1, 1)  # w / 2 for both
    ref_b, ref_1 = coef * B.grad(vs_b), R.reg_grad_v(vs_1, coef.view(-1))
    assert float((g_1.to(F64) - ref_1).abs().max()) > 1e-3  # a data term is there
    tol = (K + 4) * U * coef.abs() * B.grad_abs(vs_b) + R.tol_grad_v(ref_1, coef.view(-1), vs_1) + 2.0 * 2.0 ** -23 * torch.maximum(g_b.abs(), g_1.abs()).to(F64)
    check_each('bending/data_half', 'grad_v(bending) - grad_v(first order)', g_b.to(F64) - g_1.to(F64), ref_b - ref_1, tol)


# ------------------------------------------------------------------------------------------------------------------------------
# the frozen rule, recovery, stream capture
# ------------------------------------------------------------------------------------------------------------------------------
def pair24():
    from ir_sgmcmc_amd.data_loader import synthetic_pair
    f1, m1 = synthetic_pair((24, 24, 24), seed=0)
    return (to_dev({k: v.unsqueeze(0) for k, v in f1.items() if k != 'seg'}), to_dev({k: v.unsqueeze(0) for k, v in m1.items() if k != 'seg'}))


def bending24(seed):
    # (w_reg well inside the stability bound lr w 144 < 2 of the explicit step on the bending operator)
    return TransitionEngine(EngineConfig(dims=(24, 24, 24), seed=seed, diff_op='HessianOperator', w_reg=0.01), DEV)


def test_misprediction_is_recovered_on_a_bending_chain():
    """tests/test_gpu_transition.py::test_misprediction_is_recovered_not_fatal with the bending prior: a transition that turns out to
    be a no-op must leave v alone in the bending update too (the `frozen` rule), and irs_flush re-runs it"""
    from ir_sgmcmc_amd.ops import perturb_smooth, sobolev_kernel_1d
    N, T = 24, 6
    fixed, moving = pair24()
    v0 = perturb_smooth(torch.randn(1, 3, N, N, N, generator=torch.Generator().manual_seed(3)).to(DEV), sobolev_kernel_1d(3, 0.5))
    v0 = v0 * (9.0 / float(v0.abs().max()))
    res = {}
    for mode in (0, 3):
        eng = bending24(11)
        eng.option('predict_variants', mode)
        fd, md = eng.prepare(fixed, moving)
        eng.gmm_init(fd, md)
        v = v0.clone()
        for _ in range(T):
            eng.transition(fd, md, v)
        eng.flush()
        st = eng.state()
        assert st.iteration == T
        res[mode] = (v.clone(), list(st.gmm_log_std), eng.scalars()['reg_energy'], eng.recovered_transitions)
    assert res[0][3] == 0 and res[3][3] >= 1, (res[0][3], res[3][3])
    assert torch.equal(res[0][0], res[3][0]) and res[0][1] == res[3][1] and res[0][2] == res[3][2]
    assert not torch.equal(res[0][0], v0)


def test_captured_transition_matches_an_eager_one():
    N = 24
    fixed, moving = pair24()

    def fresh():
        eng = bending24(7)
        fd, md = eng.prepare(fixed, moving)
        eng.gmm_init(fd, md)
        return eng, fd, md

    eng, fd, md = fresh()
    v_plain = torch.zeros(1, 3, N, N, N, device=DEV)
    for _ in range(4):
        eng.transition(fd, md, v_plain)
    eng.flush()
    sc_plain = eng.scalars()

    eng, fd, md = fresh()
    v = torch.zeros(1, 3, N, N, N, device=DEV)
    eng.transition(fd, md, v)  # (lazily created resources exist before the capture)
    eng.flush()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        eng.transition(fd, md, v)
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    eng.flush()
    assert torch.equal(v, v_plain) and float(v.abs().max()) > 0.0
    assert eng.scalars()['reg_energy'] == sc_plain['reg_energy'] and int(eng.state().iteration) == 4


# ------------------------------------------------------------------------------------------------------------------------------
# autograd: the VI stage gets the prior through HIP in both directions
# ------------------------------------------------------------------------------------------------------------------------------
def test_autograd_of_a_regulariser_with_the_operator():
    """dL/dv of RegLoss_LogNormal(diff_op='HessianOperator') per element.  dL/dy reaches the kernel as a float32 number that torch
    formed from the float32 energy (cast, logarithm, the quotient by the scale twice, two sums, the quotient by y, the chain-rule
    product: 8 roundings on top of the kernel's K)."""
    from ir_sgmcmc_amd.model.loss import RegLoss_LogNormal
    from ir_sgmcmc_amd.utils.diff_op import HessianOperator
    dims, Cn = (5, 6, 7), 2
    loss = RegLoss_LogNormal(1.0, diff_op='HessianOperator', dims=dims).to(DEV)
    v0 = white((Cn, 3, *dims), 41)
    v = v0.to(DEV).requires_grad_(True)
    out, log_y = loss(v)
    out.sum().backward()
    v64 = v0.to(F64).requires_grad_(True)
    y = B._quadratic(v64, -1.0)
    loc, ls = float(loss.loc), float(loss.log_scale)
    l64 = y.log() + ls + 0.5 * ((y.log() - loc) / torch.exp(torch.tensor(ls, dtype=F64))) ** 2 + (0.5 * loss.dof - 1.0) * y.log()
    dl_dy, = torch.autograd.grad(l64.sum(), y, retain_graph=True)
    ref, = torch.autograd.grad(l64.sum(), v64)
    T = 'bending/autograd'
    check_each(T, 'loss', out.detach(), l64.detach(), 1e-5 * l64.detach().abs())
    check_each(T, 'dL/dv', v.grad, ref, (K + 8) * U * dl_dy.abs().view(-1, 1, 1, 1, 1) * B.grad_abs(v0))
    # the operator itself, (C,9,D,H,W,3): its squares sum to the same energy
    hess = HessianOperator()(v0.to(DEV))
    assert tuple(hess.shape) == (Cn, 9, *dims, 3)
    check_each(T, 'sum(HessianOperator(v)^2)', (hess.to(F64) ** 2).sum(dim=(1, 2, 3, 4, 5)), y.detach(), 1e-5 * y.detach())


# ------------------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    lib = L.load()
    cfg, ctx = irs_config(EngineConfig(dims=(16, 16, 16))), C.c_void_p()
    cfg.diff_op = 2
    assert lib.irs_create(C.byref(cfg), C.byref(ctx)) != 0 and not ctx.value
    msg = lib.irs_last_error().decode()
    assert 'diff_op' in msg and 'zero' in msg, msg
    # z-slabs: the library and the Python owner, with the same words
    cfg.diff_op = L.IRS_DIFF_HESSIAN
    scfg = L.IrsSlabConfig(0, 0)
    assert lib.irs_slab_create(C.byref(cfg), C.byref(scfg), None, C.byref(ctx)) != 0 and not ctx.value
    msg = lib.irs_last_error().decode()
    assert 'irs_slab_create' in msg and 'diff_op' in msg, msg
    from ir_sgmcmc_amd.slab import SlabEngine
    with pytest.raises(L.IrsError) as err:
        SlabEngine(EngineConfig(dims=(16, 16, 16), diff_op='HessianOperator'), DEV)
    assert str(err.value) == msg


# ------------------------------------------------------------------------------------------------------------------------------
# the trainer: baseline workload 2 cut to 24^3 and 10 transitions
# ------------------------------------------------------------------------------------------------------------------------------
def make_trainer(tmp_path, **trainer_over):
    from ir_sgmcmc_amd.parse_config import ConfigParser
    from ir_sgmcmc_amd.trainer import Trainer
    cfg = json.load(open(os.path.join(ROOT, 'configs', 'synthetic_ssd_bending_128.json')))
    cfg['trainer']['save_dir'] = str(tmp_path)
    cfg['data_loader']['args']['dims'] = [24, 24, 24]
    cfg['trainer'].update(no_iters_burn_in=4, no_samples_MCMC=6, log_period_MCMC=2, checkpoint_period=4)
    cfg['trainer'].update(trainer_over)
    config = ConfigParser.from_dict(copy.deepcopy(cfg), timestamp='t')
    dl = config.init_data_loader()
    tm, rm = config.init_transformation_and_registration_modules()
    return Trainer(config, dl, config.init_losses(), tm, rm, config.init_metrics(), device=DEV)


def digest(t):
    s = t.engine.state()
    return (t.v_curr_state.cpu(), t.displacement_mean.cpu(), t.displacement_std.cpu(), s.iteration, list(s.reg_param))


def test_trainer_runs_the_bending_config_and_resumes_bit_for_bit(tmp_path):
    a = make_trainer(tmp_path / 'a')
    assert a._engine_config().diff_op == 'HessianOperator'
    torch.manual_seed(0)
    a.run()
    a.engine.flush()
    assert bool(torch.isfinite(a.v_curr_state).all()) and float(a.v_curr_state.abs().max()) > 0.0
    # the regulariser energy the trainer logs is the engine's scalar of the last transition: the bending energy of its curr_state
    y = bending.bending_energy(a._outputs['curr_state'])
    check_each('bending/trainer', 'reg_energy of the last transition', a.engine.scalars()['reg_energy'], y, 1e-5 * y)
    assert 'MCMC/chain_0/reg/energy' in a.metrics.result()
    ck = a.config.save_dirs['checkpoints'] / 'checkpoint_0000004.pt'
    assert ck.is_file()
    b = make_trainer(tmp_path / 'b', resume=str(ck))
    torch.manual_seed(0)
    b.run()
    assert all(torch.equal(x, z) if isinstance(x, torch.Tensor) else x == z for x, z in zip(digest(a), digest(b)))
