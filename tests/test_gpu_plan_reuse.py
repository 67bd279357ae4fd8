"""Plan reuse (csrc/adjoint_plan.hip, `irs_sparse_plan_set`): the piece lists of the sparse data stage, forward steps and adjoint steps are
rebuilt only when what they are cut from changed -- the extent table of the mask (or of g_warped), the launch shape the host passes,
the per-chain dense flags -- decided on the device from a record each list keeps.  A reused list IS the list a rebuild would write,
so a chain with reuse on equals the chain with `set_sparse_plan(0)` (every list rebuilt in every transition) BIT FOR BIT: torch.equal
on v and grad_v, every scalar and state value compared as Python floats with ==  (NaN with NaN), and the three read-backs identical
after every transition.  The counters of `sparse_plan()` say which lists were rebuilt and which were kept.

Shapes (D, H, W): (72, 24, 40) and (40, 20, 70), the ragged ones of the sparse suites, every stage forced on with 8-plane pieces
(`set_sparse_data(8)`, `set_sparse_forward(8)`, the adjoint through the `march_seg` knob).  Lists per transition: the data family 3 with the
mixture loss (data term, LCC map, the warp's hull) and 1 with SSD (the hull), the forward and the adjoint family one per step."""
import gc
import struct

import pytest
import torch

from ir_sgmcmc_amd import _lib as L
from ir_sgmcmc_amd.engine import EngineConfig, TransitionEngine
from tests.test_gpu_sparse_adjoint import wave
from tests.test_gpu_sparse_data import BIG, SMALL, equal_numbers, inputs, make_mask

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PIECE = 8
REUSE, REBUILD, GRADIENT = 1, 0, 2   # irs_sparse_plan_set: reuse on / off with the default source, off with the adjoint's lists from g_warped


@pytest.fixture(autouse=True)
def pieces_of_eight():
    L.option_set('march_seg', PIECE)
    yield
    L.option_set('march_seg', 0)


def bits(x):
    """a nested list of floats / ints as exact bit patterns (-0.0 and 0.0 differ, NaN equals NaN)"""
    if hasattr(x, '__iter__'):
        return [bits(y) for y in x]
    return struct.pack('<d', float(x))


def snapshot(eng, v, grad):
    st, sc = eng.state(), eng.scalars()
    state = [list(st.gmm_log_std), list(st.gmm_logits), [list(r) for r in st.gmm_adam_m], [list(r) for r in st.gmm_adam_v],
             list(st.gmm_adam_step), list(st.reg_param), list(st.reg_adam_m), list(st.reg_adam_v), [st.iteration]]
    numbers = [sc[k] for k in sorted(sc)] + state
    return {'v': v.cpu().clone(), 'grad_v': grad.cpu().clone(), 'values': bits(numbers), 'numbers': numbers}


def run_chain(cfg, mode, images, masks, v0, *, forward=PIECE, before=None, residuals_at=(), capture_from=None):
    """transitions with masks[0], masks[1], ... under ONE mask pointer in ONE engine; before: {t: f(eng, v)} run in front of transition t;
    residuals_at: transitions that ask for the residuals; capture_from: transition t is captured and replayed from there on.
    -> per transition dict(snap, data, forward, adjoint, plan)"""
    fixed, moving = images
    eng = TransitionEngine(cfg, DEV)
    eng.set_sparse_data(PIECE)
    eng.set_sparse_forward(forward)
    eng.set_sparse_plan(mode)
    mask = masks[0].to(DEV).contiguous().clone()
    fd, md = eng.prepare({'im': fixed['im'].to(DEV), 'mask': mask}, {'im': moving['im'].to(DEV)})
    eng.gmm_init(fd, md)
    fx = {'im': fd['im'], 'mask': mask}
    v = v0.to(DEV).contiguous().clone()
    grad = torch.zeros_like(v)
    z = torch.zeros(cfg.no_chains, 1, *cfg.dims, device=DEV)
    out, graph = [], None
    for t, m in enumerate(masks):
        mask.copy_(m.to(DEV))
        if before and t in before:
            before[t](eng, v)
        outputs = {'grad_v': grad, **({'residuals': z} if t in residuals_at else {})}
        if capture_from is not None and t == capture_from:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                eng.transition(fx, md, v, outputs=outputs)
        if graph is not None:
            graph.replay()
        else:
            eng.transition(fx, md, v, outputs=outputs)
        torch.cuda.synchronize()
        out.append({'snap': snapshot(eng, v, grad), 'data': eng.sparse_data(), 'forward': eng.sparse_forward(), 'adjoint': eng.sparse_adjoint(),
                    'plan': eng.sparse_plan()})
    del graph
    return out


def assert_bit_for_bit(a, b, read_backs=('data', 'forward', 'adjoint')):
    assert len(a) == len(b)
    for t, (x, y) in enumerate(zip(a, b)):
        for key in ('v', 'grad_v'):
            assert torch.equal(x['snap'][key], y['snap'][key]), (t, key)
            assert torch.equal(torch.signbit(x['snap'][key]), torch.signbit(y['snap'][key])), (t, key, 'signs of zeros')
        assert x['snap']['values'] == y['snap']['values'], (t, x['snap']['numbers'], y['snap']['numbers'])
        for key in read_backs:
            assert x[key] == y[key], (t, key, x[key], y[key])


def per_transition(chain, family, what):
    """the counter's increments, transition by transition"""
    tot = [0] + [c['plan'][family][what] for c in chain]
    return [b - a for a, b in zip(tot, tot[1:])]


def adjoint_engaged(c):
    return [[e['engaged'] for e in step] for step in c['adjoint']]


def forward_engaged(c):
    return all(e['engaged'] == 1 for step in c['forward'] for e in step)


def expected_forward_rebuilds(chain, S):
    """list k (reach 3 S + h_{k+1} + ... + h_{n-1}) is cut again exactly when its reach is not the one it was last cut at -- with the mask,
    the options and the outputs fixed"""
    last, out = None, []
    for c in chain:
        if not forward_engaged(c):
            out.append(0)
            continue
        h = [step[0]['width'] for step in c['forward']]
        reach = [3 * S + sum(h[k + 1:]) for k in range(len(h))]
        out.append(len(h) if last is None else sum(a != b for a, b in zip(reach, last)))
        last = reach
    return out


def both(cfg, images, masks, v0, **kw):
    on = run_chain(cfg, REUSE, images, masks, v0, **kw)
    off = run_chain(cfg, REBUILD, images, masks, v0, **kw)
    assert_bit_for_bit(on, off)
    for fam in ('data', 'forward', 'adjoint'):
        assert per_transition(off, fam, 'reuses') == [0] * len(masks), (fam, off[-1]['plan'])
    return on, off


@pytest.mark.parametrize('dims,loss', [(BIG, 'GMM'), (SMALL, 'SSD')], ids=['72x24x40-GMM', '40x20x70-SSD'])
def test_constant_mask_rebuilds_once(dims, loss):
    cfg = EngineConfig(dims=dims, data_loss=loss, virtual_decimation=loss == 'GMM', lr=0.05, seed=5)
    images, v0 = inputs(dims)
    T, n, lists = 6, cfg.no_steps, 3 if loss == 'GMM' else 1
    on, off = both(cfg, images, [make_mask('ball', dims)] * T, v0)
    assert all(e == 1 for c in on for step in adjoint_engaged(c) for e in step)
    assert per_transition(on, 'data', 'rebuilds') == [lists] + [0] * (T - 1) and per_transition(on, 'data', 'reuses') == [0] + [lists] * (T - 1)
    assert per_transition(on, 'adjoint', 'rebuilds') == [n] + [0] * (T - 1) and per_transition(on, 'adjoint', 'reuses') == [0] + [n] * (T - 1)
    assert not forward_engaged(on[0]) and all(forward_engaged(c) for c in on[1:])
    expect = expected_forward_rebuilds(on, cfg.lcc_s if loss == 'GMM' else 0)
    print('forward rebuilds per transition', per_transition(on, 'forward', 'rebuilds'), 'expected', expect)
    assert per_transition(on, 'forward', 'rebuilds') == expect
    assert per_transition(on, 'forward', 'reuses') == [n - e if forward_engaged(c) else 0 for e, c in zip(expect, on)]
    assert per_transition(off, 'data', 'rebuilds') == [lists] * T and per_transition(off, 'adjoint', 'rebuilds') == [n] * T


def test_mask_sequence_under_one_pointer():
    """Rebuild, then reuse, for each new shape; clearing a voxel strictly between a column's first and last leaves the table as it is (a
    reuse), clearing the top voxel of a column does not."""
    cfg = EngineConfig(dims=BIG, lr=0.05, seed=5)
    images, v0 = inputs(BIG)
    ball, corner, shifted = (make_mask(k, BIG) for k in ('ball', 'corner_voxel', 'ball_shifted'))
    col = shifted[0, 0, :, BIG[1] // 2, BIG[2] // 2 - 10].nonzero().flatten()   # the column through the shifted ball's centre
    assert len(col) > 4
    interior, top = shifted.clone(), shifted.clone()
    interior[0, 0, int(col[len(col) // 2]), BIG[1] // 2, BIG[2] // 2 - 10] = False
    top[0, 0, int(col[-1]), BIG[1] // 2, BIG[2] // 2 - 10] = False
    on, _ = both(cfg, images, [ball, ball, corner, corner, shifted, shifted, interior, top], v0)
    changed = [1, 0, 1, 0, 1, 0, 0, 1]
    assert all(e == 1 for c in on for step in adjoint_engaged(c) for e in step)
    assert per_transition(on, 'data', 'rebuilds') == [3 * x for x in changed] and per_transition(on, 'data', 'reuses') == [3 - 3 * x for x in changed]
    assert per_transition(on, 'adjoint', 'rebuilds') == [cfg.no_steps * x for x in changed]
    fr, fu = per_transition(on, 'forward', 'rebuilds'), per_transition(on, 'forward', 'reuses')
    for t, c in enumerate(on):
        if forward_engaged(c) and changed[t]:
            assert (fr[t], fu[t]) == (cfg.no_steps, 0), (t, fr, fu)
        assert fr[t] + fu[t] == (cfg.no_steps if forward_engaged(c) else 0)
    assert on[2]['data']['data_term'][0]['run_planes'] < on[1]['data']['data_term'][0]['run_planes']


def test_dense_flip_and_back():
    """At rest, then a 3-voxel wave copied into v (the chain leaves the radius-1 kernel: full columns, the forward stage leaves), then
    the rest field again."""
    cfg = EngineConfig(dims=SMALL, lr=0.05, seed=5)
    images, v0 = inputs(SMALL)
    big = wave(SMALL, 3.0).unsqueeze(0)
    before = {3: lambda eng, v: v.copy_(big.to(DEV)), 4: lambda eng, v: v.copy_(v0.to(DEV))}
    on, _ = both(cfg, images, [make_mask('ball', SMALL)] * 8, v0, before=before)
    n = cfg.no_steps
    eng = [all(e == 1 for step in adjoint_engaged(c) for e in step) for c in on]
    print('adjoint engaged', eng, 'forward engaged', [forward_engaged(c) for c in on], 'adjoint rebuilds', per_transition(on, 'adjoint', 'rebuilds'))
    assert eng[2] and not eng[3] and eng[7]
    assert all(step[0]['engaged'] == 0 and step[0]['run_planes'] == SMALL[0] * 3 * 3 for step in on[3]['adjoint'])   # 3 x 3 tile columns, whole
    assert forward_engaged(on[2]) and not forward_engaged(on[3]) and forward_engaged(on[7])
    rb = per_transition(on, 'adjoint', 'rebuilds')
    flips = [t for t in range(1, 8) if eng[t] != eng[t - 1]]
    assert rb == [n if t == 0 or t in flips else 0 for t in range(8)]


def test_option_change_between_transitions():
    """piece length 8 -> 12 in front of transition 3: every piece list is cut again (the warp's hull has no pieces: it stays) and the
    read-backs follow"""
    cfg = EngineConfig(dims=BIG, lr=0.05, seed=5)
    images, v0 = inputs(BIG)

    def longer(eng, v):
        eng.set_sparse_data(12)
        eng.set_sparse_forward(12)
        L.option_set('march_seg', 12)

    on, _ = both(cfg, images, [make_mask('ball', BIG)] * 5, v0, before={3: longer, 0: lambda eng, v: L.option_set('march_seg', PIECE)})
    assert per_transition(on, 'data', 'rebuilds') == [3, 0, 0, 2, 0] and per_transition(on, 'adjoint', 'rebuilds') == [12, 0, 0, 12, 0]
    assert per_transition(on, 'forward', 'rebuilds')[3] == 12 and forward_engaged(on[3])
    for t, c in enumerate(on):
        want = PIECE if t < 3 else 12
        assert c['data']['data_term'][0]['piece_len'] == want and c['data']['map'][0]['piece_len'] == want
        assert all(step[0]['piece_len'] == want for step in c['adjoint'])
        assert all(step[0]['piece_len'] == want for step in c['forward']) or not forward_engaged(c)


def test_output_change_in_the_middle_of_a_chain():
    """Transition 2 asks for the residuals: the data stage is dense, the adjoint's lists come from g_warped; transition 3 cuts them from the
    mask's table again."""
    cfg = EngineConfig(dims=SMALL, lr=0.05, seed=5)
    images, v0 = inputs(SMALL)
    on, _ = both(cfg, images, [make_mask('ball', SMALL)] * 5, v0, residuals_at=(2,))
    n = cfg.no_steps
    assert all(not e['engaged'] for k in on[2]['data'] for e in on[2]['data'][k]) and not forward_engaged(on[2])
    assert per_transition(on, 'data', 'rebuilds') == [3, 0, 0, 0, 0] and per_transition(on, 'data', 'reuses') == [0, 3, 0, 3, 3]
    assert per_transition(on, 'adjoint', 'rebuilds') == [n, 0, n, n, 0]
    # the gradient's support lies inside what the mask's table promises
    assert all(on[2]['adjoint'][k][0]['run_planes'] <= on[1]['adjoint'][k][0]['run_planes'] for k in range(n))


def test_two_chains_only_one_mask_changes():
    cfg = EngineConfig(dims=SMALL, no_chains=2, lr=0.05, seed=5)
    images, v0 = inputs(SMALL, 2)
    a = torch.cat([make_mask('ball', SMALL), make_mask('cut_ball', SMALL)]).contiguous()
    b = torch.cat([make_mask('ball', SMALL), make_mask('ball_shifted', SMALL)]).contiguous()
    on, _ = both(cfg, images, [a, a, b, b, a], v0)
    assert per_transition(on, 'data', 'rebuilds') == [3, 0, 3, 0, 3] and per_transition(on, 'adjoint', 'rebuilds') == [12, 0, 12, 0, 12]
    assert on[1]['data']['warp'][0] == on[3]['data']['warp'][0] and on[1]['data']['warp'][1] != on[3]['data']['warp'][1]


def test_two_chains_share_one_mask():
    cfg = EngineConfig(dims=SMALL, no_chains=2, lr=0.05, seed=5)
    images, v0 = inputs(SMALL, 2)
    on, _ = both(cfg, images, [make_mask('ball_shifted', SMALL)] * 3 + [make_mask('ball', SMALL)], v0)
    assert per_transition(on, 'data', 'rebuilds') == [3, 0, 0, 3] and per_transition(on, 'adjoint', 'rebuilds') == [12, 0, 0, 12]
    assert all(c['data'][k][0] == c['data'][k][1] for c in on for k in ('warp', 'map', 'data_term'))


def test_captured_transition_sees_the_mask_change():
    """Transition 1 is captured and replayed; the mask changes under the pointer between replays.  Against the uncaptured chain that
    rebuilds everything (the forward steps dense in both: a captured transition plans no widths)."""
    cfg = EngineConfig(dims=SMALL, lr=0.05, seed=5)
    images, v0 = inputs(SMALL)
    masks = [make_mask(k, SMALL) for k in ('ball', 'ball', 'ball', 'ball_shifted', 'ball_shifted', 'ball')]
    on = run_chain(cfg, REUSE, images, masks, v0, forward=0, capture_from=1)
    off = run_chain(cfg, REBUILD, images, masks, v0, forward=0)
    assert_bit_for_bit(on, off)
    assert per_transition(on, 'data', 'rebuilds') == [3, 0, 0, 3, 0, 3] and per_transition(on, 'adjoint', 'rebuilds') == [12, 0, 0, 12, 0, 12]


def test_a_fresh_context_after_another_was_destroyed():
    cfg = EngineConfig(dims=SMALL, lr=0.05, seed=5)
    images, v0 = inputs(SMALL)
    masks = [make_mask('ball', SMALL)] * 2
    first = run_chain(cfg, REUSE, images, masks, v0)
    gc.collect()
    torch.cuda.synchronize()
    second = run_chain(cfg, REUSE, images, masks, v0)      # (most likely in the same memory: no record survives irs_create's clearing)
    off = run_chain(cfg, REBUILD, images, masks, v0)
    assert_bit_for_bit(first, off)
    assert_bit_for_bit(second, off)
    assert second[0]['plan'] == first[0]['plan'] and second[0]['plan']['data'] == {'rebuilds': 3, 'reuses': 0}
    assert second[0]['plan']['adjoint'] == {'rebuilds': 12, 'reuses': 0}


@pytest.mark.parametrize('dims,loss', [(BIG, 'GMM'), (SMALL, 'SSD')], ids=['72x24x40-GMM', '40x20x70-SSD'])
def test_mask_sourced_against_gradient_sourced_adjoint_lists(dims, loss):
    """Both with reuse off.  The mask's table gives a superset of the gradient's support: more planes marched, on which the gradient is
    an exact zero -- the chain is equal as numbers."""
    cfg = EngineConfig(dims=dims, data_loss=loss, virtual_decimation=loss == 'GMM', lr=0.05, seed=5)
    images, v0 = inputs(dims)
    masks = [make_mask(k, dims) for k in ('ball', 'ball', 'ball_shifted', 'ball_shifted')]
    m = run_chain(cfg, REBUILD, images, masks, v0)
    g = run_chain(cfg, GRADIENT, images, masks, v0)
    for t, (x, y) in enumerate(zip(m, g)):
        for key in ('v', 'grad_v'):
            assert equal_numbers(x['snap'][key], y['snap'][key]), (t, key)
        for p, q in zip(x['snap']['numbers'], y['snap']['numbers']):
            assert equal_numbers(p, q), (t, p, q)
        assert x['data'] == y['data'] and x['forward'] == y['forward']
        planes = [(x['adjoint'][k][0]['run_planes'], y['adjoint'][k][0]['run_planes']) for k in range(cfg.no_steps)]
        print('transition', t, 'run planes (mask, gradient) per step', planes)
        assert all(a >= b > 0 for a, b in planes), planes
        assert all(e['engaged'] == 1 for step in x['adjoint'] + y['adjoint'] for e in step)
