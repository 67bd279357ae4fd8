"""All three sparse stages on together -- the data stage (`irs_sparse_data_set`), the forward squaring steps (`irs_sparse_forward_set`)
and the adjoint squaring steps (`irs_sparse_adjoint_set`), as a new context runs them at 192^3 and above -- against all three off, in
the configurations the four sparse test files leave at their defaults: LCC half width 2 (the S = 2 instantiations of the list-walking
kernels and the reaches S, 2 S, 3 S, 3 S + sum h, 2 S + n cut for them), several chains with the data term launched per chain behind a
list-walking map (`data_on == 2`: the dense data term reads z and sigma_M over the whole volume), SVFFD (the FFD adjoint reads the
adjoint's output whole), more than four mixture components, no virtual decimation, a fixed image per chain, the unfused backward warp,
five squaring steps, a learnable log-normal regulariser and the bending prior.

What a list leaves unwritten is stale memory that only ever meets an exact zero, so the chain with the stages on EQUALS the chain with
them off as numbers (-0 == +0) after each of five transitions from the same start under production prediction: v, grad_v, every scalar,
the mixture and regulariser state.  data_term alone may differ by re-association of its fp64 sum, within the bound of
tests/test_gpu_sparse_data.py (n_mask 2^-52 |alpha| sum|-log p|, formed from the dense run's residuals); where the data term runs dense
in both chains it is the same bits.  A vacuous equality does not pass: every case asserts through the three read-backs that the lists
were walked, that the data stage's run planes are the ones the mask's geometry gives at reach 3 S / S / 2 S (S from the case), and that
the lists tests/test_sparse_configs_host.py proves strictly sparse march fewer planes than D x tile columns.  A stage that cannot
engage for a reason in the code -- the forward lists under SVFFD -- is asserted dense."""
import pytest
import torch

from ir_sgmcmc_amd import _lib as L
from ir_sgmcmc_amd.engine import EngineConfig, TransitionEngine
from tests import _sparse_configs as SC
from tests import _transition_scalars as R
from tests.test_gpu_sparse_data import assert_same_chain, inputs, make_mask, snapshot

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PIECE = 8   # pieces of at most 8 planes in all three stages: a column of the ball is cut three times


@pytest.fixture(autouse=True)
def pieces_of_eight():
    L.option_set('march_seg', 8)     # process-wide: the adjoint's piece length
    yield
    L.option_set('march_seg', 0)


def config(c):
    kw = dict(c['cfg'])
    kw.setdefault('virtual_decimation', kw.get('data_loss', 'GMM') == 'GMM')
    return EngineConfig(dims=c['dims'], no_chains=c['C'], lr=0.05, seed=5, **kw)


def case_inputs(c, cfg):
    (fixed, moving), v0 = inputs(c['dims'], c['C'])
    if cfg.cps:                      # v_0 on the control grid
        v0 = R.make_inputs(c['dims'], c['C'], amp=1.0, cps=cfg.cps)[2]
    if c['per_chain_fixed']:         # chain ch's fixed image rolled by 2 ch rows
        fixed = {'im': torch.cat([fixed['im'].roll(2 * ch, dims=-2) for ch in range(c['C'])]).contiguous()}
    return (fixed, moving), v0


def run_chain(c, on):
    """T transitions with the case's masks under ONE mask pointer in ONE engine -> (snapshot after each, the three read-backs after
    each, engine).  on: all three stages forced on with pieces of 8 planes; otherwise all three off and the residuals asked for"""
    cfg = config(c)
    (fixed, moving), v0 = case_inputs(c, cfg)
    masks = [SC.mask_of(m, c['dims']) for m in c['masks']]
    eng = TransitionEngine(cfg, DEV)
    for name, value in c['options']:
        eng.option(name, value)
    eng.set_sparse_data(PIECE if on else 0)
    eng.set_sparse_forward(PIECE if on else 0)
    eng.set_sparse_adjoint(bool(on))
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
    z = None if on else torch.zeros(cfg.no_chains, 1, *cfg.dims, device=DEV)
    snaps, plans = [], []
    for m in masks:
        mask.copy_(m.to(DEV))        # the mask changes under the same pointer
        outputs = {'grad_v': grad}
        if z is not None:
            outputs['residuals'] = z
        eng.transition(fx, md, v, outputs=outputs)
        torch.cuda.synchronize()     # (the bounds of this transition are published before the next one is planned)
        plans.append({'data': eng.sparse_data(), 'forward': eng.sparse_forward(), 'adjoint': eng.sparse_adjoint()})
        snaps.append(snapshot(eng, cfg, v, grad, z, mask))
    return snaps, plans, eng


def nothing_engaged(p):
    return all(not any(e.values()) for name in ('forward', 'adjoint') for step in p[name] for e in step) and \
           all(not any(e.values()) for rows in p['data'].values() for e in rows)


def forward_dense(p):
    return all(not any(e.values()) for step in p['forward'] for e in step)


@pytest.mark.parametrize('c', SC.CASES, ids=[c['id'] for c in SC.CASES])
def test_all_stages_on_equal_all_stages_off(c):
    cfg = config(c)
    on, plans, eng = run_chain(c, True)
    off, plans_off, eng_off = run_chain(c, False)
    assert eng.recovered_transitions == 0 and eng_off.recovered_transitions == 0
    assert all(nothing_engaged(p) for p in plans_off), plans_off
    assert_same_chain(on, off)

    D, C, n, S = c['dims'][0], c['C'], cfg.no_steps, SC.half_width(c)
    gmm, ffd = cfg.data_loss == 'GMM', cfg.cps is not None
    # the data term walks its list where one launch serves every chain; the per-chain launches keep their full columns behind a
    # list-walking map, and are then the same launches in both chains: the same bits
    one_launch = C == 1 or dict(c['options']).get('data_batch', 1) != 0
    listed = () if not gmm else ('map', 'data_term') if one_launch else ('map',)
    if gmm and not one_launch:
        assert all(a['data_term'] == b['data_term'] for a, b in zip(on, off)), [(a['data_term'], b['data_term']) for a, b in zip(on, off)]
    tot = SC.totals(c['dims'])
    for t, p in enumerate(plans):
        m = SC.mask_of(c['masks'][t], c['dims'])
        for ch in range(C):
            data, fwd, adj = {k: rows[ch] for k, rows in p['data'].items()}, [step[ch] for step in p['forward']], [step[ch] for step in p['adjoint']]
            widths = [e['width'] for e in fwd]
            print(c['id'], 'transition', t, 'chain', ch, 'data', {k: e['run_planes'] for k, e in data.items()}, 'forward', [e['run_planes'] for e in fwd],
                  'widths', widths, 'adjoint', [e['run_planes'] for e in adj], 'of', tot)
            # ---- engagement
            assert data['warp']['engaged'] == 1, p
            assert all(data[k]['engaged'] == 1 and data[k]['piece_len'] == PIECE for k in listed), p
            assert all(not any(data[k].values()) for k in ('map', 'stats', 'data_term') if k not in listed), p
            if ffd or t == 0:        # SVFFD: dense forward steps, promised; the first transition has no published bounds
                assert forward_dense(p), p
            else:
                assert all(e['engaged'] == 1 and e['piece_len'] == PIECE and e['width'] >= 1 for e in fwd), p
            assert all(e['engaged'] == 1 and e['piece_len'] == PIECE for e in adj), p
            # ---- geometry: the run planes the mask gives at each list's reach
            exp = SC.expected(m[ch if m.shape[0] > 1 else 0, 0], S, n, widths if not forward_dense(p) else None)
            assert data['warp']['run_planes'] == exp['warp'] < tot['warp'], (data, exp)
            assert all(data[k]['run_planes'] == exp[k] < tot['lcc'] for k in listed), (data, exp)
            planes = {'warp': data['warp']['run_planes'], 'map': data['map']['run_planes'], 'data_term': data['data_term']['run_planes'],
                      'adj_last': adj[n - 1]['run_planes']}
            assert [e['run_planes'] for e in adj] == exp['adjoint'], (adj, exp)
            if not forward_dense(p):
                assert [e['run_planes'] for e in fwd] == exp['forward'], (fwd, exp)
                planes.update(fwd_first=fwd[0]['run_planes'], fwd_last=fwd[n - 1]['run_planes'])
                if 'fwd_first' in c['strict']:
                    assert widths == [1] * n, widths     # (the width at which the host test proves the first list strictly sparse)
            # ---- the lists the host test proves strictly sparse
            figures = SC.strict_figures(exp, tot, n)
            for name in c['strict']:
                if name.startswith('fwd') and forward_dense(p):
                    continue
                assert 0 < planes[name] == figures[name][0] < figures[name][1], (name, planes, figures)
