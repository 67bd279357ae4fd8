"""The sparse adjoint (csrc/adjoint_plan.hip, `irs_sparse_adjoint_set`): the adjoint squaring steps march only the planes the data term's
gradient can reach and zero-fill what the next step reads around them.  Inside a run range nothing changes (the sums of a voxel run
over the same source planes in the same order whatever the cut), outside it the full-column kernel computes +-0 and the sparse path
stores +0 or leaves the voxel unread: a chain with the switch on EQUALS the chain with it off as numbers (-0 == +0), which is what
every case here asserts -- v, grad_v, the scalars and the mixture / regulariser state after each of a few transitions from the same
start, through the C ABI, every kernel variant launched (predict_variants = 0).

Shapes (D, H, W): (72, 24, 40) and (40, 20, 70) -- 2 x 3 and 3 x 3 tile columns of 32 x 8, W no multiple of 32, H no multiple of 8 --
with the piece length forced to 8 planes (`march_seg`), so that a column of the ball is cut into at least 3 pieces; 48^3 for the
displaced start of the issue.  What makes the equality mean something is asserted through the read-back: the ball engages and
marches fewer planes than D x tile columns."""
import math

import pytest
import torch

from ir_sgmcmc_amd import _lib as L
from ir_sgmcmc_amd.engine import EngineConfig, TransitionEngine
from tests import _transition_scalars as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BIG, SMALL = (72, 24, 40), (40, 20, 70)


@pytest.fixture(autouse=True)
def pieces_of_eight():
    L.option_set('march_seg', 8)
    yield
    L.option_set('march_seg', 0)


def grid(dims):
    return torch.meshgrid(*[torch.arange(n) for n in dims], indexing='ij')


def ball(dims, centre, r):
    zz, yy, xx = grid(dims)
    return (zz - centre[0]) ** 2 + (yy - centre[1]) ** 2 + (xx - centre[2]) ** 2 < r * r


def make_mask(kind, dims):
    """(1,1,D,H,W) bool"""
    D, H, W = dims
    zz, yy, xx = grid(dims)
    mid, r = ((D - 1) / 2, (H - 1) / 2, (W - 1) / 2), 0.35 * min(dims)
    if kind == 'ball':
        m = ball(dims, mid, r)
    elif kind == 'ball_shifted':        # the ball moved by 10 voxels along z and x
        m = ball(dims, (mid[0] + 10, mid[1], mid[2] - 10), r)
    elif kind == 'ones':                # every column full: the dense lists
        m = torch.ones(dims, dtype=torch.bool)
    elif kind == 'zeros':               # no run pieces at all
        m = torch.zeros(dims, dtype=torch.bool)
    elif kind == 'two_blobs':           # separated along z in the same columns: the run range is their hull
        m = ((zz >= 4) & (zz < 10) | (zz >= D - 12) & (zz < D - 6)) & (yy >= 5) & (yy < 12) & (xx >= 20) & (xx < 37)
    elif kind == 'cut_ball':            # a ball cut by three faces of the volume
        m = ball(dims, (2, 1, 3), 11)
    elif kind == 'corner_voxel':
        m = (zz == D - 1) & (yy == H - 1) & (xx == W - 1)
    return m.view(1, 1, D, H, W).contiguous()


def wave(dims, amp):
    """bench.py's 'wave' start for any dims: one half-wave across the volume, `amp` voxels"""
    s = [torch.sin(torch.linspace(0.0, math.pi, n)) for n in dims]
    w = s[0].view(-1, 1, 1) * s[1].view(1, -1, 1) * s[2].view(1, 1, -1)
    return torch.stack([w, -w, 0.7 * w]).mul(amp).contiguous()


def equal_numbers(a, b):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    return bool(((a == b) | (a.isnan() & b.isnan())).all())


def snapshot(eng, v, grad):
    st, sc = eng.state(), eng.scalars()
    state = [list(st.gmm_log_std), list(st.gmm_logits), [list(r) for r in st.gmm_adam_m], [list(r) for r in st.gmm_adam_v],
             list(st.gmm_adam_step), list(st.reg_param), list(st.reg_adam_m), list(st.reg_adam_v), [st.iteration]]
    return {'v': v.cpu().clone(), 'grad_v': grad.cpu().clone(), 'scalars': [sc[k] for k in sorted(sc)], 'state': state}


def run_chain(cfg, sparse, images, masks, v0, capture=False):
    """transitions with masks[0], masks[1], ... in ONE engine -> (snapshot after each, read-back after each)"""
    fixed, moving = images
    eng = TransitionEngine(cfg, DEV)
    eng.option('predict_variants', 0)
    if sparse is not None:              # (None: whatever a new context does)
        eng.set_sparse_adjoint(sparse)
    first = {'im': fixed['im'].to(DEV), 'mask': masks[0].to(DEV)}
    fd, md = eng.prepare(first, {'im': moving['im'].to(DEV)})
    eng.gmm_init(fd, md)
    v = v0.to(DEV).contiguous().clone()
    grad = torch.zeros_like(v)
    snaps, plans = [], []
    for i, m in enumerate(masks):
        fx = {'im': fd['im'], 'mask': m.to(DEV).contiguous()}
        if capture and i == 1:          # the second and later transitions are replays of one captured graph (same mask)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                eng.transition(fx, md, v, outputs={'grad_v': grad})
            eng._keep['captured_mask'] = fx['mask']
        if capture and i >= 1:
            g.replay()
        else:
            eng.transition(fx, md, v, outputs={'grad_v': grad})
        torch.cuda.synchronize()
        snaps.append(snapshot(eng, v, grad))
        plans.append(eng.sparse_adjoint())
    return snaps, plans


def assert_same_chain(on, off):
    assert len(on) == len(off)
    for t, (a, b) in enumerate(zip(on, off)):
        for key in ('v', 'grad_v'):
            assert torch.equal(a[key], b[key]) or equal_numbers(a[key], b[key]), (t, key, float((a[key] - b[key]).abs().max()))
        assert equal_numbers(a['scalars'], b['scalars']), (t, a['scalars'], b['scalars'])
        for x, y in zip(a['state'], b['state']):
            assert equal_numbers(x, y), (t, x, y)


def both(cfg, images, masks, v0, **kw):
    on, plans = run_chain(cfg, 1, images, masks, v0, **kw)
    off, plans_off = run_chain(cfg, 0, images, masks, v0, **kw)
    assert all(not e['engaged'] and not e['pieces'] for p in plans_off for step in p for e in step)
    assert_same_chain(on, off)
    return plans


def inputs(dims, C=1, amp=1.0):
    fixed, moving, v0, _, _ = R.make_inputs(dims, C, amp=amp)
    return (fixed, moving), v0


def tile_columns(dims):
    return ((dims[1] + 7) // 8) * ((dims[2] + 31) // 32)


CASES = [(BIG, 'GMM', 'ball'), (SMALL, 'GMM', 'ball'), (SMALL, 'SSD', 'ball'), (BIG, 'GMM', 'ones'), (SMALL, 'GMM', 'zeros'),
         (SMALL, 'SSD', 'zeros'), (BIG, 'GMM', 'two_blobs'), (SMALL, 'SSD', 'two_blobs'), (BIG, 'GMM', 'cut_ball'),
         (SMALL, 'GMM', 'cut_ball'), (BIG, 'GMM', 'corner_voxel'), (SMALL, 'SSD', 'corner_voxel')]


@pytest.mark.parametrize('dims,loss,kind', CASES, ids=['-'.join(['x'.join(map(str, c[0])), c[1], c[2]]) for c in CASES])
def test_sparse_chain_equals_the_full_column_chain(dims, loss, kind):
    cfg = EngineConfig(dims=dims, data_loss=loss, virtual_decimation=loss == 'GMM', lr=0.05, seed=5)
    images, v0 = inputs(dims)
    plans = both(cfg, images, [make_mask(kind, dims)] * 3, v0)
    n, cols, D = cfg.no_steps, tile_columns(dims), dims[0]
    for p in plans:
        assert all(p[k][0]['engaged'] == 1 and p[k][0]['piece_len'] == 8 for k in range(n)), p
        planes = [p[k][0]['run_planes'] for k in range(n)]
        assert all(planes[k] >= planes[k + 1] for k in range(n - 1)), planes   # a later step reaches one voxel further
        if kind == 'ones':
            assert planes == [D * cols] * n and all(p[k][0]['pieces'] == cols * ((D + 7) // 8) for k in range(n))
        elif kind == 'zeros':
            # nothing to march; step 0 still owes the update kernel a fully written gradient: one fill-only entry per column
            assert planes == [0] * n and [p[k][0]['pieces'] for k in range(n)] == [cols] + [0] * (n - 1), p
        else:
            assert 0 < planes[n - 1] < D * cols, planes
        if kind == 'ball':
            assert p[n - 1][0]['pieces'] >= 3   # (the first launched step: its run range alone is longer than two pieces)
            assert planes[n - 1] >= 3 * 8


def test_stale_gradient_buffers_are_refilled():
    """The gradient buffers ping-pong and keep the previous transition's values: the planes a step leaves unmarched but the next one
    reads must be zero-filled -- ball, then a single voxel (almost nothing is marched, the ball's gradient is still in the buffers),
    then the ball somewhere else."""
    cfg = EngineConfig(dims=BIG, lr=0.05, seed=5)
    images, v0 = inputs(BIG)
    masks = [make_mask(k, BIG) for k in ('ball', 'ball', 'corner_voxel', 'corner_voxel', 'ball_shifted', 'ball_shifted')]
    plans = both(cfg, images, masks, v0)
    assert all(e['engaged'] for p in plans for step in p for e in step)
    assert plans[2][11][0]['run_planes'] < plans[1][11][0]['run_planes']


def test_displaced_chain_falls_back_to_full_columns():
    """A start of 3 voxels leaves the radius-1 kernel in the late steps: the whole chain is marched densely, by whichever variant owns
    each step, and the read-back says so."""
    dims = (48, 48, 48)
    cfg = EngineConfig(dims=dims, lr=0.05, seed=5)
    images, _ = inputs(dims)
    plans = both(cfg, images, [make_mask('ball', dims)] * 3, wave(dims, 3.0).unsqueeze(0))
    for p in plans:
        assert all(step[0]['engaged'] == 0 and step[0]['run_planes'] == 48 * tile_columns(dims) for step in p), p


def test_two_chains_one_displaced_one_at_rest():
    cfg = EngineConfig(dims=SMALL, no_chains=2, lr=0.05, seed=5)
    images, _ = inputs(SMALL, 2)
    v0 = torch.stack([wave(SMALL, 3.0), torch.zeros(3, *SMALL)])
    mask = torch.cat([make_mask('ball', SMALL), make_mask('cut_ball', SMALL)]).contiguous()
    plans = both(cfg, images, [mask] * 3, v0)
    for p in plans:
        assert all(step[0]['engaged'] == 0 and step[1]['engaged'] == 1 for step in p), p
        assert p[11][1]['run_planes'] < SMALL[0] * tile_columns(SMALL)


def test_captured_transition_replays_the_sparse_chain():
    cfg = EngineConfig(dims=SMALL, lr=0.05, seed=5)
    images, v0 = inputs(SMALL)
    plans = both(cfg, images, [make_mask('ball', SMALL)] * 4, v0, capture=True)
    assert all(step[0]['engaged'] for step in plans[-1])


def test_a_new_context_marches_sparsely():
    """nobody called irs_sparse_adjoint_set: the lists are walked"""
    cfg = EngineConfig(dims=SMALL, lr=0.05, seed=5)
    images, v0 = inputs(SMALL)
    _, plans = run_chain(cfg, None, images, [make_mask('ball', SMALL)], v0)
    assert all(step[0]['engaged'] == 1 and step[0]['pieces'] > 0 for step in plans[0]), plans[0]
