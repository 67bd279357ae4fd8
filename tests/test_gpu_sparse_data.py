"""The sparse data stage (csrc/adjoint_plan.hip, `irs_sparse_data_set`): the warp computes only the tile-planes within reach of the fixed
mask, and the LCC map and the data term march piece lists around it (the data
term zero-fills the rest of g_warped).  What is skipped is only ever multiplied by an exact zero, so a chain with the switch on EQUALS
the chain with it off as numbers (-0 == +0): v, grad_v, alpha and every scalar but data_term, and the mixture / regulariser state
after each of three transitions from the same start, through the C ABI, every kernel variant launched (predict_variants = 0).
data_term[c] is an fp64 sum over the masked voxels whose grouping follows the pieces: it may differ by re-association, at most
n_masked 2^-52 relative to the sum of |-log p| (formed here in fp64 from the residuals of the dense run and the mixture after the
transition).

Shapes (D, H, W): (72, 24, 40) and (40, 20, 70) -- W no multiple of 32 or 64, H no multiple of 8 or 16, 2 x 2 and 3 x 2 tile columns of
32 x 16, 1 x 3 and 2 x 3 of 64 x 8 -- with the stage forced on and its piece length to 8 planes (`irs_sparse_data_set(ctx, 8)`), so
that a column of the ball (17 to 21 planes within reach) is cut into 3 pieces.  What makes the equality mean something is asserted through
the read-back: the ball engages and marches fewer planes than D x tile columns, "ones" marches all of them."""
import math

import pytest
import torch

from ir_sgmcmc_amd.engine import EngineConfig, TransitionEngine
from tests import _transition_scalars as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BIG, SMALL = (72, 24, 40), (40, 20, 70)
KERNELS = ('warp', 'map', 'stats', 'data_term')
SPARSE = ('warp', 'map', 'data_term')   # the kernels whose sparse form shipped


PIECE = 8   # irs_sparse_data_set(ctx, 8): on whatever the size, pieces of at most 8 planes


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
    elif kind == 'zeros':               # no run pieces at all, g_warped all fills
        m = torch.zeros(dims, dtype=torch.bool)
    elif kind == 'two_blobs':           # separated along z in the same columns: the run range is their hull
        m = ((zz >= 4) & (zz < 10) | (zz >= D - 12) & (zz < D - 6)) & (yy >= 5) & (yy < 12) & (xx >= 20) & (xx < 37)
    elif kind == 'cut_ball':            # a ball cut by three faces of the volume
        m = ball(dims, (2, 1, 3), 11)
    elif kind == 'corner_voxel':
        m = (zz == D - 1) & (yy == H - 1) & (xx == W - 1)
    return m.view(1, 1, D, H, W).contiguous()


def equal_numbers(a, b):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    return bool(((a == b) | (a.isnan() & b.isnan())).all())


def abs_nll_sum(cfg, z, mask, st):
    """sum over the masked voxels of |-log p(z)|, per chain, in fp64 (model/loss.py:87-100; SSD: 0.5 (z / sigma)^2)"""
    out = []
    for c in range(z.shape[0]):
        zc = z[c].double().flatten()[mask[c if mask.shape[0] > 1 else 0].flatten()]
        if cfg.data_loss == 'SSD':
            out.append(float((0.5 * (zc / cfg.ssd_sigma) ** 2).sum()))
            continue
        K = cfg.gmm_components
        log_std = torch.tensor(list(st.gmm_log_std)[:K], dtype=torch.float64)
        logits = torch.tensor(list(st.gmm_logits)[:K], dtype=torch.float64)
        logp = torch.logsumexp(torch.log_softmax(logits + 1e-2, 0) - log_std - 0.5 * math.log(2 * math.pi)
                               - 0.5 * (zc[:, None] * torch.exp(-log_std)) ** 2, dim=-1)
        out.append(float(logp.abs().sum()))
    return out


def snapshot(eng, cfg, v, grad, z, mask):
    st, sc = eng.state(), eng.scalars()
    state = [list(st.gmm_log_std), list(st.gmm_logits), [list(r) for r in st.gmm_adam_m], [list(r) for r in st.gmm_adam_v],
             list(st.gmm_adam_step), list(st.reg_param), list(st.reg_adam_m), list(st.reg_adam_v), [st.iteration]]
    snap = {'v': v.cpu().clone(), 'grad_v': grad.cpu().clone(), 'state': state, 'data_term': list(sc['data_term']),
            'scalars': [sc[k] for k in sorted(sc) if k != 'data_term'], 'alpha': list(sc['alpha']), 'n_mask': list(sc['n_mask'])}
    if z is not None:
        snap['abs_nll'] = abs_nll_sum(cfg, z.cpu(), mask.cpu().view(mask.shape[0], -1), st)
    return snap


def run_chain(cfg, sparse, images, masks, v0, residuals=False):
    """transitions with masks[0], masks[1], ... under ONE mask pointer in ONE engine -> (snapshot after each, read-back after each).
    residuals: the caller asks for the residuals (the dense stage, whatever the switch says)"""
    fixed, moving = images
    eng = TransitionEngine(cfg, DEV)
    eng.option('predict_variants', 0)
    eng.set_sparse_data(PIECE if sparse else 0)
    mask = masks[0].to(DEV).contiguous().clone()
    fd, md = eng.prepare({'im': fixed['im'].to(DEV), 'mask': mask}, {'im': moving['im'].to(DEV)})
    eng.gmm_init(fd, md)
    if cfg.data_loss == 'GMM' and int(masks[0].sum()) == 1:
        # One sample has no standard deviation: GMM.init_parameters leaves a NaN mixture, the whole chain turns NaN within a
        # transition, and the dense stage is NaN x 0 = NaN wherever it computes -- no statement about zeros holds there.  The
        # single-voxel mask starts from the hand-set mixture of the data-gradient tests, taken from the ball's residuals.
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
    z = torch.zeros(cfg.no_chains, 1, *cfg.dims, device=DEV) if residuals else None
    snaps, plans = [], []
    for m in masks:
        mask.copy_(m.to(DEV))            # the mask changes under the same pointer
        outputs = {'grad_v': grad}
        if residuals:
            outputs['residuals'] = z
        eng.transition(fx, md, v, outputs=outputs)
        torch.cuda.synchronize()
        snaps.append(snapshot(eng, cfg, v, grad, z, mask))
        plans.append(eng.sparse_data())
    return snaps, plans


def assert_same_chain(on, off):
    """`off` ran the dense stage with the residuals asked for: it carries sum |-log p|"""
    assert len(on) == len(off)
    for t, (a, b) in enumerate(zip(on, off)):
        for key in ('v', 'grad_v'):
            assert torch.equal(a[key], b[key]) or equal_numbers(a[key], b[key]), (t, key, float((a[key] - b[key]).abs().max()))
        assert equal_numbers(a['scalars'], b['scalars']), (t, a['scalars'], b['scalars'])
        for x, y in zip(a['state'], b['state']):
            assert equal_numbers(x, y), (t, x, y)
        for c, (x, y) in enumerate(zip(a['data_term'], b['data_term'])):
            tol = b['n_mask'][c] * 2.0 ** -52 * abs(b['alpha'][c]) * b['abs_nll'][c]
            print('transition', t, 'chain', c, 'data_term', x, y, 'difference', abs(x - y), 'bound', tol)
            assert equal_numbers([x], [y]) or abs(x - y) <= tol, (t, c, x, y, tol)   # (an empty mask: NaN both)


def nothing_engaged(plans):
    return all(not e['engaged'] and not e['run_planes'] for p in plans for k in KERNELS for e in p[k])


def both(cfg, images, masks, v0):
    on, plans = run_chain(cfg, 1, images, masks, v0)
    off, plans_off = run_chain(cfg, 0, images, masks, v0, residuals=True)
    assert nothing_engaged(plans_off)
    assert_same_chain(on, off)
    return plans


def inputs(dims, C=1, amp=1.0):
    fixed, moving, v0, _, _ = R.make_inputs(dims, C, amp=amp)
    return (fixed, moving), v0


def columns(dims, tile):
    return ((dims[1] + tile[1] - 1) // tile[1]) * ((dims[2] + tile[0] - 1) // tile[0])


def run_lengths(mask, tile, reach):
    """Per tile column of `tile` = (tx, ty) the planes within `reach` (Chebyshev) of the mask (D,H,W), as a hull along z: what the
    device plan must have found -- formed here from the mask's geometry alone"""
    D, H, W = mask.shape
    has = mask.any(0)
    zz = torch.arange(D).view(D, 1, 1)
    lo = torch.where(mask, zz, D).amin(0)
    hi = torch.where(mask, zz + 1, 0).amax(0)
    out = []
    for y0 in range(0, H, tile[1]):
        for x0 in range(0, W, tile[0]):
            win = (slice(max(y0 - reach, 0), min(y0 + tile[1] + reach, H)), slice(max(x0 - reach, 0), min(x0 + tile[0] + reach, W)))
            if not bool(has[win].any()):
                out.append((0, 0))
                continue
            out.append((max(int(lo[win][has[win]].min()) - reach, 0), min(int(hi[win][has[win]].max()) + reach, D)))
    return out


def planes_of(ranges):
    return sum(b - a for a, b in ranges)


CASES = [(BIG, 'GMM', 'ball'), (SMALL, 'GMM', 'ball'), (SMALL, 'SSD', 'ball'), (BIG, 'GMM', 'ball_shifted'), (BIG, 'GMM', 'ones'),
         (SMALL, 'SSD', 'ones'), (SMALL, 'GMM', 'zeros'), (SMALL, 'SSD', 'zeros'), (BIG, 'GMM', 'two_blobs'), (SMALL, 'SSD', 'two_blobs'),
         (BIG, 'GMM', 'cut_ball'), (SMALL, 'GMM', 'cut_ball'), (BIG, 'GMM', 'corner_voxel'), (SMALL, 'SSD', 'corner_voxel')]


@pytest.mark.parametrize('dims,loss,kind', CASES, ids=['-'.join(['x'.join(map(str, c[0])), c[1], c[2]]) for c in CASES])
def test_sparse_stage_equals_the_dense_stage(dims, loss, kind):
    cfg = EngineConfig(dims=dims, data_loss=loss, virtual_decimation=loss == 'GMM', lr=0.05, seed=5)
    images, v0 = inputs(dims)
    plans = both(cfg, images, [make_mask(kind, dims)] * 3, v0)
    D, lcc_cols, warp_cols = dims[0], columns(dims, (32, 16)), columns(dims, (64, 8))
    listed = ('map', 'data_term') if loss == 'GMM' else ()
    for p in plans:
        assert all(p[k][0]['engaged'] == 1 for k in ('warp',) + listed), p
        # (the statistics keep their dense launch: trimming their segments measured no faster -- the record says so)
        assert all(p[k][0]['engaged'] == 0 and p[k][0]['run_planes'] == 0 for k in KERNELS if k not in ('warp',) + listed), p
        assert all(p[k][0]['piece_len'] == 8 for k in listed), p
        planes = {k: p[k][0]['run_planes'] for k in KERNELS}
        if kind == 'ones':
            assert planes['warp'] == D * warp_cols and all(planes[k] == D * lcc_cols for k in listed), planes
            assert all(p[k][0]['pieces'] == lcc_cols * ((D + 7) // 8) for k in listed), p
        elif kind == 'zeros':
            # nothing to march; the data term still owes the adjoint a fully written g_warped: one fill entry per column
            assert planes['warp'] == 0 and all(planes[k] == 0 for k in listed), planes
            if listed:
                assert p['map'][0]['pieces'] == 0 and p['data_term'][0]['pieces'] == lcc_cols, p
        else:
            assert 0 < planes['warp'] < D * warp_cols, planes
            assert all(0 < planes[k] < D * lcc_cols for k in listed), planes
            if listed:
                assert planes['map'] <= planes['data_term']    # reach s inside reach 2 s
        # the run ranges are the ones the mask's geometry gives (reach: 3 s / s / 2 s around the LCC map, the mask itself for SSD)
        m3 = make_mask(kind, dims)[0, 0]
        assert planes['warp'] == planes_of(run_lengths(m3, (64, 8), 3 if loss == 'GMM' else 0)), planes
        if listed:
            dt = run_lengths(m3, (32, 16), 2)
            assert planes['map'] == planes_of(run_lengths(m3, (32, 16), 1)) and planes['data_term'] == planes_of(dt), planes
            # run pieces of 8 planes at most, a fill below and above the run range where it does not touch the volume's end
            assert p['data_term'][0]['pieces'] == sum((b - a + 7) // 8 + ((a > 0) + (b < D) if b > a else 1) for a, b in dt), p
            if kind == 'ball':
                assert max(b - a for a, b in dt) > 16   # a column of the ball is cut at least 3 times


def test_the_mask_changes_under_the_same_pointer():
    """The extents are found in every transition, and g_warped keeps the previous transition's values where the mask has been: ball,
    then a single voxel (almost nothing is marched, the ball's gradient is still in the buffer and must be filled over), then the
    ball somewhere else (z, sigma_M and the warped image around it are two transitions old or were never written)."""
    cfg = EngineConfig(dims=BIG, lr=0.05, seed=5)
    images, v0 = inputs(BIG)
    masks = [make_mask(k, BIG) for k in ('ball', 'corner_voxel', 'ball_shifted')]
    plans = both(cfg, images, masks, v0)
    assert all(p[k][0]['engaged'] for p in plans for k in SPARSE)
    assert plans[1]['data_term'][0]['run_planes'] < plans[0]['data_term'][0]['run_planes']
    assert plans[1]['warp'][0]['run_planes'] < plans[2]['warp'][0]['run_planes']


@pytest.mark.parametrize('loss', ['GMM', 'SSD'])
def test_two_chains_with_their_own_masks(loss):
    cfg = EngineConfig(dims=SMALL, no_chains=2, data_loss=loss, lr=0.05, seed=5)
    images, v0 = inputs(SMALL, 2)
    mask = torch.cat([make_mask('ball', SMALL), make_mask('cut_ball', SMALL)]).contiguous()
    plans = both(cfg, images, [mask] * 3, v0)
    for p in plans:
        assert all(p[k][c]['engaged'] == 1 for k in (SPARSE if loss == 'GMM' else ('warp',)) for c in range(2)), p
        assert p['warp'][0]['run_planes'] != p['warp'][1]['run_planes']
        assert all(0 < p['warp'][c]['run_planes'] < SMALL[0] * columns(SMALL, (64, 8)) for c in range(2))


def test_two_chains_share_one_mask():
    cfg = EngineConfig(dims=SMALL, no_chains=2, lr=0.05, seed=5)
    images, v0 = inputs(SMALL, 2)
    plans = both(cfg, images, [make_mask('ball_shifted', SMALL)] * 3, v0)
    for p in plans:
        assert all(p[k][0] == p[k][1] and p[k][0]['engaged'] == 1 for k in SPARSE), p


def test_a_caller_who_asks_for_the_residuals_gets_the_dense_stage():
    cfg = EngineConfig(dims=SMALL, lr=0.05, seed=5)
    images, v0 = inputs(SMALL)
    masks = [make_mask('ball', SMALL)] * 3
    on, plans = run_chain(cfg, 1, images, masks, v0, residuals=True)
    off, _ = run_chain(cfg, 0, images, masks, v0, residuals=True)
    assert nothing_engaged(plans)
    assert_same_chain(on, off)
    assert all(a['data_term'] == b['data_term'] for a, b in zip(on, off))   # the same launches: the same bits


def test_a_new_context_runs_the_sparse_stage_where_the_size_rule_lets_it():
    """Nobody called irs_sparse_data_set.  On the small volume the full-column LCC launches already use the shortest pieces: the dense
    stage runs.  (120, 256, 256) is the smallest volume of 256 x 256 planes whose full-column segments are longer than the shortest
    piece (128 tile columns x 15 segments of 8 planes are more than a resident set of the map): the lists are walked, with a piece
    length the plan chose.  Inputs made on the device, one transition."""
    cfg = EngineConfig(dims=SMALL, lr=0.05, seed=5)
    images, v0 = inputs(SMALL)
    eng = TransitionEngine(cfg, DEV)
    fd, md = eng.prepare({'im': images[0]['im'].to(DEV), 'mask': make_mask('ball', SMALL).to(DEV)}, {'im': images[1]['im'].to(DEV)})
    eng.gmm_init(fd, md)
    eng.transition(fd, md, v0.to(DEV).contiguous().clone())
    assert nothing_engaged([eng.sparse_data()])
    del eng
    dims = (120, 256, 256)
    zz, yy, xx = [torch.linspace(-1, 1, n, device=DEV).view(*[-1 if i == a else 1 for i in range(3)]) for a, n in enumerate(dims)]
    fixed = (torch.sin(7 * xx) * torch.cos(5 * yy + 2 * zz) + 0.3 * torch.sin(23 * xx * yy + 11 * zz)).view(1, 1, *dims).contiguous()
    moving = (torch.sin(7 * xx + 0.1) * torch.cos(5 * yy + 2 * zz - 0.1) + 0.3 * torch.sin(23 * xx * yy + 11 * zz + 0.2)).view(1, 1, *dims).contiguous()
    mask = (xx * xx + yy * yy + zz * zz < 0.5).view(1, 1, *dims).contiguous()
    eng = TransitionEngine(EngineConfig(dims=dims, lr=0.05, seed=5), DEV)
    fd, md = eng.prepare({'im': fixed, 'mask': mask}, {'im': moving})
    eng.gmm_init(fd, md)
    eng.transition(fd, md, torch.zeros(1, 3, *dims, device=DEV))
    plan = eng.sparse_data()
    assert all(plan[k][0]['engaged'] == 1 and plan[k][0]['run_planes'] > 0 for k in SPARSE), plan
    assert all(8 <= plan[k][0]['piece_len'] <= 64 for k in ('map', 'data_term')), plan
    assert plan['warp'][0]['run_planes'] < 120 * columns(dims, (64, 8)) and plan['data_term'][0]['run_planes'] < 120 * columns(dims, (32, 16))
    sc = eng.scalars()
    assert math.isfinite(sc['data_term'][0]) and sc['n_mask'][0] == float(mask.sum())
