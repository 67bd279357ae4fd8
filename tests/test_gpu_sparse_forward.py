"""The sparse forward squaring steps (csrc/adjoint_plan.hip, `irs_sparse_forward_set`): step k computes d_{k+1} only on the run pieces of
its list -- per 64 x 8 tile column the planes within 3 S + h_{k+1} + ... + h_{n-1} voxels of the fixed mask, h_i the width the host
planned for step i from the published bounds -- which is where the warp, the steps behind it and the adjoint read it.  What is skipped
is stale but finite and only ever meets a zero weight or a zero gradient, so a chain with the switch on EQUALS the chain with it off
as numbers (-0 == +0): v, grad_v, every scalar (data_term included: the forward pass regroups no sum) and the mixture / regulariser
state after every transition.  The widths are in the transition's verdict: a plan that does not hold makes the transition a no-op
that is re-run dense.

Shapes (D, H, W): (72, 24, 40) and (40, 20, 70) -- W no multiple of 64, H no multiple of 8, 1 x 3 and 2 x 3 tile columns of 64 x 8 --
with the stage forced on and its piece length to 8 planes (and the data stage with it: its extent table is what the lists are cut
from).  The first transition of a context has no published bounds and runs dense; the later ones must engage, which is asserted
through the read-back together with what makes the equalities mean something: the ball marches fewer planes than D x tile columns
("At D = 72 the ball with the widest reach spans 47 of the 72 planes"), "ones" marches all of them."""
import math

import pytest
import torch

from ir_sgmcmc_amd.engine import EngineConfig, TransitionEngine
from tests import _transition_scalars as R
from tests.test_gpu_sparse_data import BIG, SMALL, columns, equal_numbers, inputs, make_mask

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PIECE = 8   # irs_sparse_forward_set(ctx, 8) / irs_sparse_data_set(ctx, 8): on whatever the size, pieces of at most 8 planes
T = 5       # transitions per chain: the first is dense (no bounds published yet), four engage


def snapshot(eng, v, grad):
    st, sc = eng.state(), eng.scalars()
    state = [list(st.gmm_log_std), list(st.gmm_logits), [list(r) for r in st.gmm_adam_m], [list(r) for r in st.gmm_adam_v],
             list(st.gmm_adam_step), list(st.reg_param), list(st.reg_adam_m), list(st.reg_adam_v), [st.iteration]]
    return {'v': v.cpu().clone(), 'grad_v': grad.cpu().clone(), 'state': state, 'scalars': [sc[k] for k in sorted(sc)]}


def run_chain(cfg, forward, images, masks, v0, *, options=(), outputs=(), data=PIECE):
    """transitions with masks[0], masks[1], ... under ONE mask pointer in ONE engine -> (snapshot after each, read-back after each,
    engine).  forward / data: the arguments of irs_sparse_forward_set / irs_sparse_data_set (None: the call is not made).  outputs:
    names of further outputs the caller asks for."""
    fixed, moving = images
    eng = TransitionEngine(cfg, DEV)
    for name, value in options:
        eng.option(name, value)
    if data is not None:
        eng.set_sparse_data(data)
    if forward is not None:
        eng.set_sparse_forward(forward)
    mask = masks[0].to(DEV).contiguous().clone()
    fd, md = eng.prepare({'im': fixed['im'].to(DEV), 'mask': mask}, {'im': moving['im'].to(DEV)})
    eng.gmm_init(fd, md)
    if cfg.data_loss == 'GMM' and int(masks[0].sum()) == 1:
        # (one sample has no standard deviation -- tests/test_gpu_sparse_data.py: run_chain; the hand-set mixture of the ball instead)
        st = eng.state()
        ls, lg = R.hand_set_mixture({'im': fixed['im'], 'mask': make_mask('ball', cfg.dims)}, {'im': moving['im']}, cfg.gmm_components, cfg.lcc_s)
        for k in range(cfg.gmm_components):
            st.gmm_log_std[k], st.gmm_logits[k] = float(ls[k]), float(lg[k])
            for i in range(2):
                st.gmm_adam_m[i][k] = st.gmm_adam_v[i][k] = 0.0
        st.gmm_adam_step[0] = st.gmm_adam_step[1] = 0
        eng.set_state(st)
    fx = {'im': fd['im'], 'mask': mask}
    v = v0.to(DEV).contiguous().clone()
    grad = torch.zeros_like(v)
    extra = {name: torch.zeros(cfg.no_chains, 1 if name == 'residuals' else 3, *cfg.dims, device=DEV) for name in outputs}
    snaps, plans = [], []
    for m in masks:
        mask.copy_(m.to(DEV))            # the mask changes under the same pointer
        eng.transition(fx, md, v, outputs={'grad_v': grad, **extra})
        torch.cuda.synchronize()         # (the bounds of this transition are published before the next one is planned)
        plans.append(eng.sparse_forward())
        snaps.append(snapshot(eng, v, grad))
    return snaps, plans, eng


def assert_same_chain(on, off):
    assert len(on) == len(off)
    for t, (a, b) in enumerate(zip(on, off)):
        for key in ('v', 'grad_v'):
            assert torch.equal(a[key], b[key]) or equal_numbers(a[key], b[key]), (t, key, float((a[key] - b[key]).abs().max()))
        for x, y in zip(a['scalars'], b['scalars']):
            assert equal_numbers(x, y), (t, x, y)
        for x, y in zip(a['state'], b['state']):
            assert equal_numbers(x, y), (t, x, y)


def engaged(plan):
    return all(e['engaged'] == 1 and e['piece_len'] == PIECE and e['width'] >= 1 for step in plan for e in step)


def nothing_engaged(plans):
    return all(not any(e.values()) for p in plans for step in p for e in step)


def both(cfg, images, masks, v0, **kw):
    on, plans, eng = run_chain(cfg, PIECE, images, masks, v0, **kw)
    off, plans_off, _ = run_chain(cfg, 0, images, masks, v0, **kw)
    assert nothing_engaged(plans_off)
    assert_same_chain(on, off)
    return plans, eng


CASES = [(BIG, 'GMM', 'ball'), (SMALL, 'SSD', 'ball'), (SMALL, 'GMM', 'ball_shifted'), (BIG, 'GMM', 'two_blobs'), (SMALL, 'GMM', 'cut_ball'),
         (BIG, 'GMM', 'corner_voxel'), (BIG, 'GMM', 'ones'), (SMALL, 'SSD', 'ones'), (SMALL, 'SSD', 'zeros')]


@pytest.mark.parametrize('dims,loss,kind', CASES, ids=['-'.join(['x'.join(map(str, c[0])), c[1], c[2]]) for c in CASES])
def test_sparse_steps_equal_the_dense_steps(dims, loss, kind):
    cfg = EngineConfig(dims=dims, data_loss=loss, virtual_decimation=loss == 'GMM', lr=0.05, seed=5)
    images, v0 = inputs(dims)
    plans, eng = both(cfg, images, [make_mask(kind, dims)] * T, v0)
    assert eng.recovered_transitions == 0
    D, cols, n = dims[0], columns(dims, (64, 8)), cfg.no_steps
    assert nothing_engaged(plans[:1])          # no bounds published yet: dense
    for p in plans[1:]:
        assert engaged(p), p
        planes = [p[k][0]['run_planes'] for k in range(n)]
        print(kind, 'run planes per step', planes, 'of', D * cols, 'widths', [p[k][0]['width'] for k in range(n)])
        assert all(planes[k] >= planes[k + 1] for k in range(n - 1)), planes       # the reach shrinks towards the warp
        if kind == 'ones':
            assert all(x == D * cols for x in planes), planes
            assert all(p[k][0]['pieces'] == cols * ((D + PIECE - 1) // PIECE) for k in range(n)), p
        elif kind == 'zeros':
            assert all(x == 0 for x in planes) and all(p[k][0]['pieces'] == 0 for k in range(n)), p
        else:
            assert all(0 < x for x in planes), planes
            if kind in ('ball', 'ball_shifted', 'corner_voxel'):
                assert planes[0] < D * cols, planes
        if kind == 'ball' and dims == BIG:
            # every tile column is within reach of the ball's longest column: its planes, and 3 S + h_1 + ... + h_11 >= 14 either side
            nz = int(make_mask(kind, dims)[0, 0].any(-1).any(-1).sum())
            assert cols * (nz + 2 * (3 + n - 1)) <= planes[0] < D * cols, (planes, nz)


def test_the_mask_moves_under_the_same_pointer():
    """ball -> ball_shifted between transitions: the planes the second ball needs and the first did not hold values that are several
    transitions old, or were never written sparsely.  They must be computed, not left."""
    cfg = EngineConfig(dims=BIG, lr=0.05, seed=5)
    images, v0 = inputs(BIG)
    masks = [make_mask(k, BIG) for k in ('ball', 'ball', 'ball', 'ball_shifted', 'ball_shifted', 'ball')]
    plans, eng = both(cfg, images, masks, v0)
    assert eng.recovered_transitions == 0
    assert all(engaged(p) for p in plans[1:]), plans


@pytest.mark.parametrize('loss', ['GMM', 'SSD'])
def test_two_chains_with_their_own_masks(loss):
    cfg = EngineConfig(dims=SMALL, no_chains=2, data_loss=loss, lr=0.05, seed=5)
    images, v0 = inputs(SMALL, 2)
    mask = torch.cat([make_mask('ball', SMALL), make_mask('cut_ball', SMALL)]).contiguous()
    plans, eng = both(cfg, images, [mask] * T, v0)
    assert eng.recovered_transitions == 0
    for p in plans[1:]:
        assert engaged(p), p
        assert p[cfg.no_steps - 1][0]['run_planes'] != p[cfg.no_steps - 1][1]['run_planes']     # each chain its own lists
        assert all(0 < p[cfg.no_steps - 1][c]['run_planes'] < SMALL[0] * columns(SMALL, (64, 8)) for c in range(2))


def half_wave(dims, peak):
    """a smooth half-wave of `peak` voxels at the volume's centre -- inside the ball -- falling to zero at the faces, on every axis"""
    zz, yy, xx = [torch.sin(math.pi * (torch.arange(n) + 0.5) / n).view(*[-1 if i == a else 1 for i in range(3)]) for a, n in enumerate(dims)]
    w = (zz * yy * xx).view(1, 1, *dims)
    return (peak * torch.cat([w, -w, w], 1)).contiguous()


PEAK = 2.5   # voxels: d_11 is half the smoothed velocity, max|d_11| about 1.2 -- beyond one voxel, below the 1.5 of the any-radius adjoint


def test_a_step_of_width_two():
    cfg = EngineConfig(dims=BIG, lr=0.05, seed=5)
    images, _ = inputs(BIG)
    n = cfg.no_steps
    plans, eng = both(cfg, images, [make_mask('ball', BIG)] * T, half_wave(BIG, PEAK))
    assert eng.recovered_transitions == 0          # floor(max|d_11|) + 1 <= 2 held in every transition ...
    for p in plans[1:]:
        assert engaged(p), p
        assert p[n - 1][0]['width'] == 2, p        # ... with the width planned from a bound beyond 0.6 voxel
        assert all(p[k][0]['width'] == 1 for k in range(n - 2)), p


def test_a_wrong_plan_is_caught_and_repaired():
    """The same start with every planned width forced to 1 (slab_force_h on a context without a slab): max|d_11| is beyond one voxel, so
    floor(max|d_11|) + 1 = 2 > 1 -- the device finds the plan violated, the transition is a no-op, and it is re-run dense.  That
    max|d_11| really is beyond one voxel is what the failure shows (test_a_step_of_width_two: no failure at width 2).  The tile body
    clamps every tap into the volume, so the dropped transition read nothing out of bounds."""
    cfg = EngineConfig(dims=BIG, lr=0.05, seed=5)
    images, _ = inputs(BIG)
    masks, v0 = [make_mask('ball', BIG)] * 6, half_wave(BIG, PEAK)
    wrong, plans, eng = run_chain(cfg, PIECE, images, masks, v0, options=(('slab_force_h', 1),))
    assert any(engaged(p) and all(e['width'] == 1 for step in p for e in step) for p in plans), plans
    assert eng.recovered_transitions >= 1
    plain, plans_plain, ref = run_chain(cfg, PIECE, images, masks, v0, options=(('predict_variants', 0),))
    assert nothing_engaged(plans_plain) and ref.recovered_transitions == 0
    # (the snapshots were taken through state(), which flushes: every transition happened exactly once, dense)
    for t, (a, b) in enumerate(zip(wrong, plain)):
        assert torch.equal(a['v'], b['v']) and torch.equal(a['grad_v'], b['grad_v']), t
        assert a['state'] == b['state'] and a['scalars'] == b['scalars'], t


@pytest.mark.parametrize('why', ['transformation', 'displacement', 'residuals', 'predict_variants', 'default'])
def test_dense_where_promised(why):
    cfg = EngineConfig(dims=SMALL, lr=0.05, seed=5)
    images, v0 = inputs(SMALL)
    masks = [make_mask('ball', SMALL)] * 4
    # (a default-constructed engine: nobody calls either switch, and at this size the rule on sizes keeps both stages dense)
    kw = {'outputs': (why,)} if why in ('transformation', 'displacement', 'residuals') else \
         {'options': (('predict_variants', 0),)} if why == 'predict_variants' else {'data': None}
    on, plans, _ = run_chain(cfg, None if why == 'default' else PIECE, images, masks, v0, **kw)
    assert nothing_engaged(plans), plans
    off, _, _ = run_chain(cfg, 0, images, masks, v0, **kw)
    assert_same_chain(on, off)
