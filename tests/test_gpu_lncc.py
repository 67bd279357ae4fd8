"""The LNCC data term on the GPU (csrc/lncc_kernels.hip) against the float64 restatement of tests/_lncc.py, whose tolerance is derived
there: the two operators element by element, g_warped inside a transition read through grad_v, the default path left alone,
recovery and stream capture, the autograd layer, the refusals and the trainer.

Geometry of the two kernels: a workgroup owns a 32 x 8 column tile with a halo of r voxels and marches a z segment with a run-in of
r planes on either side; by size a segment is at least 4 r planes long (`lcc_seg` forces a length).  The shapes (D,H,W) in those terms:
  (3,3,3)     the smallest legal volume at r = 1: one tile, every window clamps on all six faces, both folds meet in one voxel's taps;
  (5,9,129)   four full x tiles and one 1 voxel wide, a full tile row and a 1-row one; r = 1: segments 3 + 2; r = 2: the smallest depth,
              one segment whose run-in is clamped planes only;
  (7,13,70)   two full x tiles and a 6-wide one, a 5-row last tile row; r = 1: segments 4 + 3, r = 2: one of 7;
  (9,9,9), (9,17,33) at r = 4: the widest window, 16 x 40 staged per plane, the window as large as the volume in (9,9,9);
  (12,8,64)   exact multiples of the tile: every halo beyond the last tile lies outside the volume; r = 1: segments of exactly 4;
  (11,13,70)  three chains, segments 4 + 4 + 3;
  lcc_seg = 2: segments shorter than the window (r = 1: 2 < 3, r = 2: 2 < 5) -- a ring that is primed by run-in planes alone."""
import contextlib
import copy
import ctypes as C
import gc
import json
import math
import os

import pytest
import torch

from ir_sgmcmc_amd import _lib as L
from ir_sgmcmc_amd import lncc
from ir_sgmcmc_amd.engine import EngineConfig, TransitionEngine, irs_config
from tests import _data_gradient as G
from tests import _lncc as N
from tests._report import check

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F64 = torch.float64
U = N.U
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def name(dims, *rest):
    return '-'.join(['x'.join(map(str, dims))] + [str(r) for r in rest])


def check_each(test, key, a, b, tol):
    """|a - b| <= tol element by element; the parity report gets the worst deviation in units of its tolerance"""
    a, b, tol = (torch.as_tensor(x, dtype=F64).cpu() for x in (a, b, tol))
    exact = (a == b) | (a.isnan() & b.isnan())
    dev = torch.where(exact, torch.zeros_like(a), (a - b).abs() / tol)
    print(f'{test}: {key}: worst deviation / tolerance {float(dev.max()):.4f}')
    return check(test, key + ' [deviation / tolerance]', dev, torch.zeros_like(dev), 1.0)


def to_dev(d):
    return {k: v.to(DEV).contiguous() for k, v in d.items()}


@contextlib.contextmanager
def lcc_seg(n):
    """the process-wide segment length of the LCC / LNCC kernels; it may only change while no context is alive"""
    gc.collect()
    if n:
        L.option_set('lcc_seg', n)
    try:
        yield
    finally:
        gc.collect()
        if n:
            L.option_set('lcc_seg', 0)


# ------------------------------------------------------------------------------------------------------------------------------
# the two stateless operators
# ------------------------------------------------------------------------------------------------------------------------------
OPS_CASES = [
    # dims, r, C, fixed per chain, upstream (None | 'shared' | 'per_chain'), lcc_seg
    ((3, 3, 3), 1, 1, False, None, 0),
    ((5, 9, 129), 1, 2, False, None, 0), ((5, 9, 129), 2, 2, True, 'shared', 0),
    ((7, 13, 70), 1, 2, True, 'per_chain', 0), ((7, 13, 70), 2, 2, False, 'shared', 0),
    ((9, 9, 9), 4, 1, False, None, 0), ((9, 17, 33), 4, 2, True, 'per_chain', 0),
    ((12, 8, 64), 1, 2, False, 'per_chain', 0), ((12, 8, 64), 2, 1, False, None, 0),
    ((11, 13, 70), 1, 3, True, 'per_chain', 0), ((11, 13, 70), 3, 3, False, 'per_chain', 0),
    ((7, 13, 70), 2, 2, False, 'per_chain', 2), ((11, 13, 70), 1, 3, True, 'shared', 2),
]


def ops_inputs(dims, Cn, per_chain_fixed, upstream):
    """white-noise images (texture in every window), the moving image correlated with the fixed one; the upstream weight has entries
    of both signs"""
    gen = torch.Generator().manual_seed(7)
    fixed = torch.rand(Cn if per_chain_fixed else 1, 1, *dims, generator=gen)
    moving = (0.6 * fixed + 0.7 * torch.rand(Cn, 1, *dims, generator=gen)).contiguous()
    u = None if upstream is None else torch.randn(Cn if upstream == 'per_chain' else 1, 1, *dims, generator=gen)
    return fixed, moving, u


@pytest.mark.parametrize('dims,r,Cn,per_chain_fixed,upstream,seg', OPS_CASES, ids=[name(*c) for c in OPS_CASES])
def test_operators_per_element(dims, r, Cn, per_chain_fixed, upstream, seg):
    fixed, moving, u = ops_inputs(dims, Cn, per_chain_fixed, upstream)
    fd, md, ud = fixed.to(DEV), moving.to(DEV), None if u is None else u.to(DEV)
    with lcc_seg(seg):
        out = lncc.lncc_forward(fd, md, r, N.EPS, ud)
        g = lncc.lncc_backward(fd, md, out['coef'], r)
        again = lncc.lncc_forward(fd, md, r, N.EPS, ud)
        g_again = lncc.lncc_backward(fd, md, again['coef'], r)
        sums2, g2 = lncc.lncc_loss(fd, md, r, N.EPS, ud)
        single = []
        for c in range(Cn):
            fc = fd[c:c + 1] if per_chain_fixed else fd
            uc = None if ud is None else (ud[c:c + 1] if ud.shape[0] > 1 else ud)
            oc = lncc.lncc_forward(fc, md[c:c + 1], r, N.EPS, uc)
            single.append((oc, lncc.lncc_backward(fc, md[c:c + 1], oc['coef'], r)))
    ref = N.reference(fixed, moving, 1.0 if u is None else u, r)
    T = 'lncc/operators/' + name(dims, r, Cn, per_chain_fixed, upstream, seg)
    assert out['d'].dtype == torch.float32 and out['sums'].dtype == F64 and tuple(out['coef'].shape) == (Cn, 3, *dims)
    assert float(ref['g'].abs().max()) > 1e-3
    check_each(T, 'd', out['d'], ref['d'], ref['tol']['d'])
    for j, k in enumerate('pqt'):
        check_each(T, k, out['coef'][:, j:j + 1], ref[k], ref['tol'][k])
    check_each(T, 'g', g, ref['g'], ref['tol']['g'])
    check_each(T, 'sums', out['sums'], ref['sums'], ref['tol']['sums'])
    # no atomics, a fixed order of every sum: the same bits again, and chain c of the batch is the single-chain call
    for k in ('d', 'coef', 'sums'):
        assert torch.equal(out[k], again[k]), k
    assert torch.equal(g, g_again) and torch.equal(g, g2) and torch.equal(out['sums'], sums2)
    for c, (oc, gc_) in enumerate(single):
        for k in ('d', 'coef', 'sums'):
            assert torch.equal(out[k][c:c + 1], oc[k]), (k, c)
        assert torch.equal(g[c:c + 1], gc_), c


def test_flat_window_and_optional_outputs():
    """no special case: a flat fixed image gives d = 1 and gradient 0 (den = eps); outputs that are not asked for are not written"""
    dims = (6, 9, 40)
    fixed = torch.full((1, 1, *dims), 0.25, device=DEV)
    moving = torch.rand(2, 1, *dims, generator=torch.Generator().manual_seed(1)).to(DEV)
    out = lncc.lncc_forward(fixed, moving, 1)
    assert float((out['d'] - 1.0).abs().max()) < 1e-3 and float(lncc.lncc_backward(fixed, moving, out['coef'], 1).abs().max()) < 1e-2
    only = lncc.lncc_forward(fixed, moving, 1, want_map=False, want_coef=False)
    assert only['d'] is None and only['coef'] is None and torch.equal(only['sums'], out['sums'])


def test_wrapper_checks():
    f, m = torch.rand(1, 1, 6, 7, 8).to(DEV), torch.rand(2, 1, 6, 7, 8).to(DEV)
    with pytest.raises(L.IrsError, match='radius'):
        lncc.lncc_forward(f, m, 0)
    with pytest.raises(L.IrsError, match='radius'):
        lncc.lncc_forward(f, m, 5)
    with pytest.raises(L.IrsError, match='2 radius'):
        lncc.lncc_forward(f, m, 3)
    with pytest.raises(L.IrsError, match='eps'):
        lncc.lncc_forward(f, m, 1, eps=0.0)
    with pytest.raises(L.IrsError, match='does not match'):
        lncc.lncc_forward(f, m, 1, upstream=torch.ones(3, 1, 6, 7, 8, device=DEV))
    with pytest.raises(L.IrsError, match='coef'):
        lncc.lncc_backward(f, m, torch.zeros(2, 2, 6, 7, 8, device=DEV), 1)
    with pytest.raises(L.IrsError, match='float32'):
        lncc.lncc_forward(f, m.double(), 1)
    with pytest.raises(L.IrsError, match='GPU only'):
        lncc.lncc_forward(f.cpu(), m.cpu(), 1)


# ------------------------------------------------------------------------------------------------------------------------------
# g_warped inside a transition, read through grad_v at velocity zero (tests/_data_gradient.py): grad_v[ch] = g_M Delta_ch m
# ------------------------------------------------------------------------------------------------------------------------------
A_, B_, E_, M_ = G.DYADIC
WEIGHT = 3.0
ENGINE_CASES = [
    # dims, r, C, mask ('ones' | 'band'), per-chain fixed image
    (A_, 1, 1, 'ones', False), (A_, 2, 1, 'band', False), (B_, 1, 1, 'band', False), (B_, 2, 1, 'ones', False),
    (E_, 1, 1, 'ones', False), (E_, 2, 1, 'band', False), (M_, 2, 1, 'ones', False), (M_, 1, 3, 'band', True),
    (A_, 1, 3, 'ones', True), (E_, 2, 3, 'ones', False),
]


def engine_inputs(dims, Cn, mask_kind, per_chain_fixed):
    fixed, _ = G.smooth_fixed(dims, Cn if per_chain_fixed else 1)
    D = dims[0]
    mask = torch.ones(1, 1, *dims, dtype=torch.bool)
    if mask_kind == 'band':   # a few planes around D / 2: g_warped is zero beyond r planes of them, the sparse adjoint's support
        mask[:, :, :max(D // 2 - 1, 0)] = False
        mask[:, :, D // 2 + 1:] = False
    return fixed, G.tri_image(dims), mask.contiguous()


def engine_config(dims, r, Cn, **kw):
    return EngineConfig(dims=dims, no_chains=Cn, sobolev_s=0, uniform_noise=0.0, lcc_s=r, lr=0.05, data_loss='LNCC', virtual_decimation=False,
                        lncc_weight=WEIGHT, **kw)


def run_engine(case, sparse_adjoint=None):
    dims, r, Cn, mask_kind, per_chain_fixed = case
    fixed, moving, mask = engine_inputs(dims, Cn, mask_kind, per_chain_fixed)
    eng = TransitionEngine(engine_config(dims, r, Cn), DEV)
    try:
        eng.option('predict_variants', 0)   # every kernel variant is launched: nothing is assumed, no transition is re-run
        if sparse_adjoint is not None:
            eng.set_sparse_adjoint(sparse_adjoint)
        fd, md = eng.prepare(to_dev({'im': fixed, 'mask': mask}), to_dev({'im': moving}))
        nan = lambda *shape: torch.full(shape, float('nan'), device=DEV, dtype=torch.float32)
        out = {'curr_state': nan(Cn, 3, *dims), 'residuals': nan(Cn, 1, *dims), 'grad_v': nan(Cn, 3, *dims), 'displacement': nan(Cn, 3, *dims)}
        v = torch.zeros(Cn, 3, *dims, device=DEV)
        eng.transition(fd, md, v, None, torch.zeros(Cn, 3, *dims, device=DEV), None, out)
        sc = eng.scalars()
        res = {k: t.cpu() for k, t in out.items()}
        res.update(scalars=sc, v_new=v.cpu(), engaged=max(e['engaged'] for step in eng.sparse_adjoint() for e in step))
        return res
    finally:
        eng.__del__()


def hold(case, res, tag=''):
    dims, r, Cn, mask_kind, per_chain_fixed = case
    fixed, moving, mask = engine_inputs(dims, Cn, mask_kind, per_chain_fixed)
    T = 'lncc/transition/' + name(*case) + tag
    assert int(torch.count_nonzero(res['displacement'])) == 0 and int(torch.count_nonzero(res['curr_state'])) == 0
    grad, d = res['grad_v'], res['residuals']
    assert bool(torch.isfinite(grad).all()) and bool(torch.isfinite(d).all())
    u = mask.to(F64)
    ref = N.reference(fixed, moving, u, r, scale=WEIGHT)
    full = lambda t: t.expand(Cn, -1, -1, -1, -1)
    check_each(T, 'residuals = d', d, full(ref['d']), full(ref['tol']['d']))
    sc = res['scalars']
    assert sc['alpha'] == [1.0] * Cn and sc['n_mask'] == [float(mask.sum())] * Cn
    check_each(T, 'data_term', sc['data_term'], ref['sums'].expand(Cn), ref['tol']['sums'].expand(Cn))
    dm = G.one_sided_differences(moving[0, 0].to(F64)).unsqueeze(0)       # (1,3,D,H,W)
    g_ref, tol_g = full(ref['g']), full(ref['tol']['g'])
    assert float(g_ref.abs().max()) > 1e-3
    # the read-out's own rounding, the 8-tap cancellation of the warp adjoint: 8 U max|m| / |Delta m| relative (tests/_data_gradient.py)
    tol = tol_g * dm.abs() + 8.0 * U * float(moving.abs().max()) * g_ref.abs() * (dm != 0).to(F64)
    for ch, ax in enumerate((-1, -2, -3)):
        assert int(torch.count_nonzero(grad[:, ch].narrow(ax, 0, 1))) == 0 and int(torch.count_nonzero(grad[:, ch].narrow(ax, dims[ax] - 1, 1))) == 0
        check_each(T, f'grad_v channel {ch}', grad[:, ch], (g_ref * dm)[:, ch], tol[:, ch])
    assert torch.equal(res['v_new'], -(torch.tensor(0.05, dtype=torch.float32) * grad))


@pytest.mark.parametrize('case', ENGINE_CASES, ids=[name(*c) for c in ENGINE_CASES])
def test_g_warped_in_a_transition(case):
    hold(case, run_engine(case))


@pytest.fixture
def short_adjoint_pieces():
    L.option_set('march_seg', 8)     # process-wide: the adjoint's piece length, so that lists exist on volumes this small
    yield
    L.option_set('march_seg', 0)


@pytest.mark.parametrize('case', [(E_, 2, 1, 'band', False), (M_, 1, 3, 'band', True)], ids=lambda c: name(*c))
def test_sparse_adjoint_does_not_change_a_bit(case, short_adjoint_pieces):
    on, off = run_engine(case), run_engine(case, sparse_adjoint=False)
    hold(case, on, '-sparse_adjoint')
    assert on['engaged'] == 1 and off['engaged'] == 0
    for k in ('grad_v', 'residuals', 'v_new'):
        assert torch.equal(on[k], off[k]), k
    assert on['scalars'] == off['scalars']


def test_weight_and_eps_travel_through_irs_lncc_set():
    """data_term and grad_v scale with the weight; another eps gives another d"""
    case = (A_, 1, 1, 'ones', False)
    dims, r, Cn = case[:3]
    fixed, moving, mask = engine_inputs(dims, Cn, case[3], case[4])
    res = {}
    for w, eps in ((1.0, 1e-5), (4.0, 1e-5), (1.0, 1e-2)):
        eng = TransitionEngine(EngineConfig(dims=dims, sobolev_s=0, uniform_noise=0.0, lcc_s=r, lr=0.05, data_loss='LNCC',
                                            virtual_decimation=False, lncc_weight=w, lncc_eps=eps), DEV)
        fd, md = eng.prepare(to_dev({'im': fixed, 'mask': mask}), to_dev({'im': moving}))
        out = {'grad_v': torch.empty(1, 3, *dims, device=DEV), 'residuals': torch.empty(1, 1, *dims, device=DEV)}
        eng.transition(fd, md, torch.zeros(1, 3, *dims, device=DEV), None, torch.zeros(1, 3, *dims, device=DEV), None, out)
        res[(w, eps)] = (eng.scalars()['data_term'][0], out['grad_v'].cpu(), out['residuals'].cpu())
        eng.__del__()
    (t1, g1, d1), (t4, g4, d4), (_, _, d_eps) = res[(1.0, 1e-5)], res[(4.0, 1e-5)], res[(1.0, 1e-2)]
    assert t4 == 4.0 * t1 and torch.equal(g4, 4.0 * g1) and torch.equal(d4, d1)     # (a power of two: exact)
    assert not torch.equal(d_eps, d1)
    ref = N.terms(fixed, moving, 1.0, r, eps=1e-2)['d']
    check_each('lncc/transition/eps', 'd at eps = 1e-2', d_eps, ref, N.tolerance(fixed, moving, 1.0, r, eps=1e-2)['d'])


# ------------------------------------------------------------------------------------------------------------------------------
# the default path: a context with the new data loss in the process changes nothing for the others
# ------------------------------------------------------------------------------------------------------------------------------
def pair24():
    from ir_sgmcmc_amd.data_loader import synthetic_pair
    f1, m1 = synthetic_pair((24, 24, 24), seed=0)
    return (to_dev({k: v.unsqueeze(0) for k, v in f1.items() if k != 'seg'}), to_dev({k: v.unsqueeze(0) for k, v in m1.items() if k != 'seg'}))


def lncc24(seed, **kw):
    return TransitionEngine(EngineConfig(dims=(24, 24, 24), seed=seed, data_loss='LNCC', lcc_s=2, virtual_decimation=False, lncc_weight=10.0, **kw), DEV)


def chain(eng, fixed, moving, T=3):
    fd, md = eng.prepare(fixed, moving)
    if eng.cfg.data_loss == 'GMM':
        eng.gmm_init(fd, md)
    v = torch.zeros(eng.cfg.no_chains, 3, 24, 24, 24, device=DEV)
    for _ in range(T):
        eng.transition(fd, md, v)
    eng.flush()
    return v.clone(), eng.scalars()


def test_default_path_unchanged():
    fixed, moving = pair24()
    cfgs = [EngineConfig(dims=(24, 24, 24), seed=5), EngineConfig(dims=(24, 24, 24), seed=5, data_loss='SSD', virtual_decimation=False)]
    before = [chain(TransitionEngine(c, DEV), fixed, moving) for c in cfgs]
    v_l, sc_l = chain(lncc24(5), fixed, moving)
    assert bool(torch.isfinite(v_l).all()) and not torch.equal(v_l, before[1][0])
    after = [chain(TransitionEngine(c, DEV), fixed, moving) for c in cfgs]
    for (v0, s0), (v1, s1) in zip(before, after):
        assert torch.equal(v0, v1) and s0 == s1 and float(v0.abs().max()) > 0.0


# ------------------------------------------------------------------------------------------------------------------------------
# the frozen rule, recovery, stream capture (tests/test_gpu_bending.py)
# ------------------------------------------------------------------------------------------------------------------------------
def test_misprediction_is_recovered_on_an_lncc_chain():
    from ir_sgmcmc_amd.ops import perturb_smooth, sobolev_kernel_1d
    Nn, T = 24, 6
    fixed, moving = pair24()
    v0 = perturb_smooth(torch.randn(1, 3, Nn, Nn, Nn, generator=torch.Generator().manual_seed(3)).to(DEV), sobolev_kernel_1d(3, 0.5))
    v0 = v0 * (9.0 / float(v0.abs().max()))
    res = {}
    for mode in (0, 3):
        eng = lncc24(11)
        eng.option('predict_variants', mode)
        fd, md = eng.prepare(fixed, moving)
        v = v0.clone()
        for _ in range(T):
            eng.transition(fd, md, v)
        eng.flush()
        assert eng.state().iteration == T
        sc = eng.scalars()
        res[mode] = (v.clone(), sc['data_term'], sc['reg_energy'], eng.recovered_transitions)
    assert res[0][3] == 0 and res[3][3] >= 1, (res[0][3], res[3][3])
    assert torch.equal(res[0][0], res[3][0]) and res[0][1] == res[3][1] and res[0][2] == res[3][2]
    assert not torch.equal(res[0][0], v0) and math.isfinite(res[0][1][0])


def test_captured_transition_matches_an_eager_one():
    Nn = 24
    fixed, moving = pair24()

    def fresh():
        eng = lncc24(7)
        fd, md = eng.prepare(fixed, moving)
        return eng, fd, md

    eng, fd, md = fresh()
    v_plain = torch.zeros(1, 3, Nn, Nn, Nn, device=DEV)
    for _ in range(4):
        eng.transition(fd, md, v_plain)
    eng.flush()
    sc_plain = eng.scalars()

    eng, fd, md = fresh()
    v = torch.zeros(1, 3, Nn, Nn, Nn, device=DEV)
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
    sc = eng.scalars()
    assert sc['data_term'] == sc_plain['data_term'] and sc['reg_energy'] == sc_plain['reg_energy'] and int(eng.state().iteration) == 4


# ------------------------------------------------------------------------------------------------------------------------------
# autograd: model.loss.LNCC runs the two HIP operators in both directions
# ------------------------------------------------------------------------------------------------------------------------------
def test_autograd_of_the_loss_class():
    from ir_sgmcmc_amd.model.loss import DataLoss, LNCC
    dims, Cn, r, w = (5, 6, 7), 2, 2, 3.0
    loss = LNCC(radius=r, weight=w)
    assert isinstance(loss, DataLoss) and loss.no_components == 1
    gen = torch.Generator().manual_seed(9)
    fixed = torch.rand(1, 1, *dims, generator=gen)
    moving = (0.6 * fixed + 0.7 * torch.rand(Cn, 1, *dims, generator=gen)).contiguous()
    wgt = torch.randn(Cn, 1, *dims, generator=gen)      # what sits between the map and the loss: any weights, negative ones too
    m = moving.to(DEV).requires_grad_(True)
    z = loss.map(fixed.to(DEV).expand(Cn, -1, -1, -1, -1), m)
    total = loss(z * wgt.to(DEV))
    total.backward()
    u = torch.tensor(w, dtype=torch.float32) * wgt      # the upstream gradient as the backward receives it, float32
    ref = N.reference(fixed, moving, u, r)
    T = 'lncc/autograd'
    check_each(T, 'map', z.detach(), ref['d'], ref['tol']['d'])
    check_each(T, 'loss', total.detach(), ref['sums'].sum(), 1e-5 * ref['tol']['sums'].sum() / N.LOSS_RTOL)
    check_each(T, 'dL/dM', m.grad, ref['g'], ref['tol']['g'])
    auto = N.autograd_gradient(fixed, moving, u, r)
    assert float((ref['g'] - auto).abs().max()) <= 1e-12 * float(auto.abs().max())
    # the masked form the VI stage uses: loss(map[mask])
    mask = torch.rand(Cn, 1, *dims, generator=gen) > 0.3
    m2 = moving.to(DEV).requires_grad_(True)
    loss(loss.map(fixed.to(DEV), m2)[mask.to(DEV)]).backward()
    ref2 = N.reference(fixed, moving, w * mask.to(F64), r)
    check_each(T, 'dL/dM, masked', m2.grad, ref2['g'], ref2['tol']['g'])


# ------------------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------------------
def refused(lib, cfg):
    ctx = C.c_void_p()
    assert lib.irs_create(C.byref(cfg), C.byref(ctx)) != 0 and not ctx.value
    return lib.irs_last_error().decode()


def test_refusals():
    lib = L.load()
    base = dict(dims=(16, 16, 16), data_loss='LNCC', lcc_s=2, virtual_decimation=False)
    assert 'virtual decimation' in refused(lib, irs_config(EngineConfig(**{**base, 'virtual_decimation': True})))
    for r in (0, 5):
        msg = refused(lib, irs_config(EngineConfig(**{**base, 'lcc_s': r})))
        assert 'LNCC radius' in msg and '1..4' in msg, msg
    msg = refused(lib, irs_config(EngineConfig(**{**base, 'dims': (16, 4, 16)})))
    assert 'every dim >= 5' in msg, msg
    cfg = irs_config(EngineConfig(**base))
    cfg.data_loss = 2       # reserved
    assert refused(lib, cfg) == 'irs_create: unknown data loss'
    # z-slabs: the library and the Python owner, with the same words
    cfg, ctx, scfg = irs_config(EngineConfig(**base)), C.c_void_p(), L.IrsSlabConfig(0, 0)
    assert lib.irs_slab_create(C.byref(cfg), C.byref(scfg), None, C.byref(ctx)) != 0 and not ctx.value
    msg = lib.irs_last_error().decode()
    assert 'irs_slab_create' in msg and 'LNCC' in msg, msg
    from ir_sgmcmc_amd.slab import SlabEngine
    with pytest.raises(L.IrsError) as err:
        SlabEngine(EngineConfig(**base), DEV)
    assert str(err.value) == msg
    with pytest.raises(ValueError, match='data_loss'):
        irs_config(EngineConfig(dims=(16, 16, 16), data_loss='NCC'))


def test_lncc_set_refusals():
    eng = lncc24(1)
    for w, e in ((0.0, 1e-5), (float('nan'), 1e-5), (1.0, 0.0), (1.0, float('nan')), (float('inf'), 1e-5), (-1.0, 1e-5)):
        with pytest.raises(L.IrsError, match='finite values > 0'):
            eng.lncc_set(w, e)
    eng.lncc_set(2.0, 1e-4)     # before the first transition: fine
    fixed, moving = pair24()
    fd, md = eng.prepare(fixed, moving)
    eng.transition(fd, md, torch.zeros(1, 3, 24, 24, 24, device=DEV))
    eng.flush()
    with pytest.raises(L.IrsError, match='only before the first transition'):
        eng.lncc_set(2.0, 1e-4)
    other = TransitionEngine(EngineConfig(dims=(24, 24, 24), data_loss='SSD', virtual_decimation=False), DEV)
    with pytest.raises(L.IrsError, match='not IRS_DATA_LNCC'):
        other.lncc_set(1.0, 1e-5)
    with pytest.raises(L.IrsError, match='finite values > 0'):
        TransitionEngine(EngineConfig(dims=(24, 24, 24), data_loss='LNCC', lcc_s=1, virtual_decimation=False, lncc_weight=0.0), DEV)


# ------------------------------------------------------------------------------------------------------------------------------
# the trainer: the new config cut to 24^3 and ten transitions
# ------------------------------------------------------------------------------------------------------------------------------
def make_trainer(tmp_path, top=None, **trainer_over):
    from ir_sgmcmc_amd.parse_config import ConfigParser
    from ir_sgmcmc_amd.trainer import Trainer
    cfg = json.load(open(os.path.join(ROOT, 'configs', 'synthetic_lncc_l2_128.json')))
    cfg['trainer']['save_dir'] = str(tmp_path)
    cfg['data_loader']['args']['dims'] = [24, 24, 24]
    cfg['trainer'].update(no_iters_burn_in=4, no_samples_MCMC=6, log_period_MCMC=2, checkpoint_period=4)
    cfg['trainer'].update(trainer_over)
    cfg.update(top or {})
    config = ConfigParser.from_dict(copy.deepcopy(cfg), timestamp='t')
    dl = config.init_data_loader()
    tm, rm = config.init_transformation_and_registration_modules()
    return Trainer(config, dl, config.init_losses(), tm, rm, config.init_metrics(), device=DEV)


def digest(t):
    s = t.engine.state()
    return (t.v_curr_state.cpu(), t.displacement_mean.cpu(), t.displacement_std.cpu(), s.iteration, list(s.reg_param))


def test_trainer_runs_the_config_and_resumes_bit_for_bit(tmp_path):
    a = make_trainer(tmp_path / 'a')
    ec = a._engine_config()
    cfg = json.load(open(os.path.join(ROOT, 'configs', 'synthetic_lncc_l2_128.json')))['data_loss']['args']
    assert (ec.data_loss, ec.lcc_s, ec.lncc_weight, ec.lncc_eps) == ('LNCC', cfg['radius'], cfg['weight'], cfg['eps'])
    torch.manual_seed(0)
    a.run()
    a.engine.flush()
    assert bool(torch.isfinite(a.v_curr_state).all()) and float(a.v_curr_state.abs().max()) > 0.0
    res = a.metrics.result()
    assert math.isfinite(res['MCMC/chain_0/data_term']) and res['MCMC/chain_0/data_term'] > 0.0
    # the data term the trainer logs is weight * sum mask (1 - cc) of the last warped image
    out = lncc.lncc_forward(a._fixed['im'], a._outputs['im_moving_warped'], ec.lcc_s, ec.lncc_eps, a._fixed['mask'].to(torch.float32))
    check_each('lncc/trainer', 'data_term of the last transition', a.engine.scalars()['data_term'], ec.lncc_weight * out['sums'],
               1e-5 * ec.lncc_weight * out['sums'].abs())
    ck = a.config.save_dirs['checkpoints'] / 'checkpoint_0000004.pt'
    assert ck.is_file()
    b = make_trainer(tmp_path / 'b', resume=str(ck))
    torch.manual_seed(0)
    b.run()
    assert all(torch.equal(x, z) if isinstance(x, torch.Tensor) else x == z for x, z in zip(digest(a), digest(b)))


def test_trainer_vi_stage_runs_with_the_class(tmp_path):
    t = make_trainer(tmp_path, VI=True, MCMC=False, no_iters_VI=2, no_samples_VI_test=1, log_period_VI=1)
    t.run()
    res = t.metrics.result()
    assert t.metrics._count['VI/train/data_term'] == 2 and math.isfinite(res['VI/train/data_term']) and res['VI/train/data_term'] > 0.0
    assert math.isfinite(res['VI/train/total_loss'])


def test_trainer_refusals(tmp_path):
    with pytest.raises(ValueError, match='virtual decimation'):
        make_trainer(tmp_path / 'a', top={'virtual_decimation': True})._engine_config()
    with pytest.raises(ValueError, match='residual_check'):
        make_trainer(tmp_path / 'b', residual_check={'bins': 32})._engine_config()
