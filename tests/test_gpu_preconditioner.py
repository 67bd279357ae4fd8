"""The adaptive preconditioner on the GPU: both operators through their wrappers against the numpy restatement
(tests/_preconditioner.py), the refusals of the C ABI, and the trainer option.

The second moment and the sigma field are compared bit for bit.  The two means are double sums of N = 3 n non-negative terms
whose order differs between the device and numpy: each of the two carries an error of at most (N - 1) 2^-53 of the sum, so
the tests allow a difference of N 2^-52 of the value.  Gbar is compared with the restatement's sum of the G formed with the
device's sbar (lambda is rounded to float32, so the last bits of sbar can move every G), and the field with the restatement given
both of the device's means."""
import copy
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from ir_sgmcmc_amd import _lib as L
from ir_sgmcmc_amd import preconditioner as P
from ir_sgmcmc_amd.engine import TransitionEngine
from tests import _preconditioner as S

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# below one tile; ragged with 3 n no multiple of 4; an extent below 2 r + 1 at r = 2 and x beyond one 64-wide tile
GRIDS = [(5, 6, 7), (9, 17, 33), (3, 4, 67)]
CHAINS = [1, 2, 3]
f32 = np.float32

dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
bits = lambda x: x.view(torch.int32)


def gradients(C_, grid, seed, steps=5):
    """`steps` gradient fields whose magnitude varies over four decades across the volume"""
    rng = np.random.default_rng(seed)
    scale = np.exp(rng.uniform(-4.0, 4.0, (1, 3, *grid)))
    return [(rng.standard_normal((C_, 3, *grid)) * scale).astype(f32) for _ in range(steps)]


def accumulated(C_, grid, seed, beta=0.9):
    """(the wrapper's state, the restatement's V) after five updates without a sigma field"""
    state, V = P.preconditioner_state(grid, DEV), np.zeros((1, 3, *grid), f32)
    for g in gradients(C_, grid, seed):
        P.preconditioner_accumulate(dev(g), None, state, beta)
        V, _ = S.accumulate(V, g, None, beta)
    return state, V


# ---------------------------------------------------------------- accumulate
@pytest.mark.parametrize('grid', GRIDS)
@pytest.mark.parametrize('C_', CHAINS)
@pytest.mark.parametrize('mode', ['none', 'ones', 'random'])
def test_accumulate_is_the_restatement_bit_for_bit(grid, C_, mode):
    rng = np.random.default_rng(3)
    sigma = {'none': None, 'ones': np.ones((C_, 3, *grid), f32),
             'random': rng.uniform(0.25, 4.0, (C_, 3, *grid)).astype(f32)}[mode]
    state, V = P.preconditioner_state((C_, 3, *grid), DEV), np.zeros((1, 3, *grid), f32)
    assert state['V'].shape == (1, 3, *grid) and state['count'] == 0 and int(state['nonfinite']) == 0
    plain = P.preconditioner_state(grid, DEV)
    for t, g in enumerate(gradients(C_, grid, 11), 1):
        P.preconditioner_accumulate(dev(g), None if sigma is None else dev(sigma), state, 0.9)
        V, bad = S.accumulate(V, g, sigma, 0.9)
        assert bad == 0 and state['count'] == t
        assert state['V'].cpu().numpy().tobytes() == V.tobytes(), f'update {t}'
        if mode == 'ones':  # the same bits as no sigma field at all
            P.preconditioner_accumulate(dev(g), None, plain, 0.9)
            assert torch.equal(bits(plain['V']), bits(state['V']))
    assert int(state['nonfinite']) == 0 and float(state['V'].min()) > 0.0


def test_accumulate_counts_non_finite_gradients():
    grid, C_ = (9, 17, 33), 2
    g = gradients(C_, grid, 2, steps=1)[0]
    g[1, 2, 8, 16, 32], g[0, 0, 0, 0, 0], g[0, 1, 4, 4, 4] = np.nan, np.inf, -np.inf
    state = P.preconditioner_state(grid, DEV)
    P.preconditioner_accumulate(dev(g), None, state, 0.9)
    P.preconditioner_accumulate(dev(np.abs(g)), None, state, 0.9)
    assert int(state['nonfinite']) == 6  # added to, call after call
    V = state['V'].cpu().numpy()
    assert (~np.isfinite(V)).sum() == 3 and not np.isfinite(V[0, 2, 8, 16, 32])
    sigma, summary = P.preconditioner_sigma(state, C_, 0.9)  # nothing crashes; the counter is in the summary
    torch.cuda.synchronize()
    assert summary['nonfinite'] == 6 and sigma.shape == (C_, 3, *grid)


# ---------------------------------------------------------------- sigma
@pytest.mark.parametrize('grid', GRIDS)
@pytest.mark.parametrize('r', [0, 1, 2])
@pytest.mark.parametrize('C_', CHAINS)
def test_sigma_is_the_restatement(grid, r, C_):
    state, V = accumulated(C_, grid, 7)
    assert state['V'].cpu().numpy().tobytes() == V.tobytes()
    args = dict(smooth=r, damping=0.1, sigma_min=0.875, sigma_max=1.125)  # a clamp both ends of every one of these fields reach
    sigma, got = P.preconditioner_sigma(state, C_, 0.9, **args)
    N, bias = V.size, S.bias_correction(0.9, 5)
    sbar, _ = S.means(V, bias, r, 0.1)
    _, gbar = S.means(V, bias, r, 0.1, sbar=got['s_mean'])
    print(f'grid {grid} r {r} C {C_}: sbar {got["s_mean"]!r} / {sbar!r}, Gbar {got["G_mean"]!r} / {gbar!r}, bound {N * 2.0 ** -52:.3g} relative')
    assert abs(got['s_mean'] - sbar) <= N * 2.0 ** -52 * sbar
    assert abs(got['G_mean'] - gbar) <= N * 2.0 ** -52 * gbar
    want, summary = S.sigma_field(V, C_, bias, r, 0.1, 0.875, 1.125, sbar=got['s_mean'], gbar=got['G_mean'])
    assert sigma.cpu().numpy().tobytes() == want.tobytes()
    for key in ('sigma_min', 'sigma_max', 'clamped_low', 'clamped_high', 'nonfinite'):
        assert got[key] == summary[key], key
    assert got['clamped_low'] > 0 and got['clamped_high'] > 0 and (got['sigma_min'], got['sigma_max']) == (0.875, 1.125)
    assert abs(got['sigma2_mean'] - summary['sigma2_mean']) <= N * 2.0 ** -52 * summary['sigma2_mean']
    for c in range(1, C_):  # the C copies are one field
        assert torch.equal(bits(sigma[c]), bits(sigma[0]))
    # the same call again, and the same sequence from scratch: the same bits, the summary's doubles included
    again, got2 = P.preconditioner_sigma(state, C_, 0.9, **args)
    fresh, got3 = P.preconditioner_sigma(accumulated(C_, grid, 7)[0], C_, 0.9, **args)
    assert torch.equal(bits(again), bits(sigma)) and torch.equal(bits(fresh), bits(sigma)) and got2 == got and got3 == got


def test_sigma_before_any_gradient_is_one():
    state = P.preconditioner_state((5, 6, 7), DEV)
    for r in (0, 2):
        sigma, got = P.preconditioner_sigma(state, 2, 0.99, smooth=r)
        assert (sigma == 1.0).all() and got['s_mean'] == 0.0 and got['G_mean'] == 1.0 and got['sigma2_mean'] == 1.0
        assert got['clamped_low'] == got['clamped_high'] == got['nonfinite'] == 0


def test_exact_case_on_the_device():
    """|g| = 2^k, beta = 1/2: V_t = g^2 (1 - 2^-t) and sigma = 1 in every bit (tests/test_preconditioner_host.py has the reasoning)"""
    grid = (9, 17, 33)
    state = P.preconditioner_state(grid, DEV)
    rng = np.random.default_rng(1)
    for t in range(1, 6):
        g = np.where(rng.random((3, 3, *grid)) < 0.5, -8.0, 8.0).astype(f32)
        P.preconditioner_accumulate(dev(g), None, state, 0.5)
        assert (state['V'] == 64.0 * (1.0 - 2.0 ** -t)).all()
        for r in (0, 1, 2):
            sigma, got = P.preconditioner_sigma(state, 3, 0.5, smooth=r)
            assert (sigma == 1.0).all() and got['sigma2_mean'] == 1.0


# ---------------------------------------------------------------- the C ABI refuses what it cannot do
def test_abi_refusals():
    lib = L.load()
    grid, C_ = (5, 6, 7), 2
    n3 = 3 * 5 * 6 * 7
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    grad = torch.ones(C_, 3, *grid, device=DEV)
    sg = torch.ones(C_, 3, *grid, device=DEV)
    V = torch.full((1, 3, *grid), 7.0, device=DEV)
    count = torch.zeros(1, device=DEV, dtype=torch.int64)
    out = torch.full((C_, 3, *grid), 7.0, device=DEV)
    summary = torch.full((L.IRS_PRECOND_SUMMARY,), 7.0, device=DEV, dtype=torch.float64)
    nbytes = C.c_size_t()
    assert lib.irs_precond_workspace(*grid, 2, C.byref(nbytes)) == 0 and nbytes.value > 4 * n3
    ws = torch.empty(nbytes.value, device=DEV, dtype=torch.uint8)
    small = C.c_size_t()
    assert lib.irs_precond_workspace(*grid, 0, C.byref(small)) == 0 and small.value == nbytes.value - 4 * n3

    def acc(g=grad, s=sg, Cn=C_, d=grid, beta=0.9, v=V, cnt=count):
        return lib.irs_precond_accumulate(p(g), p(s), Cn, *d, beta, p(v), p(cnt), None)

    def sig(v=V, Cn=C_, d=grid, bias=1.5, r=2, damping=0.1, lo=0.25, hi=4.0, cnt=count, o=out, sm=summary, w=ws, wb=None):
        return lib.irs_precond_sigma(p(v), Cn, *d, bias, r, damping, lo, hi, p(cnt), p(o), p(sm), p(w),
                                     nbytes.value if wb is None else wb, None)

    A, G = 'irs_precond_accumulate', 'irs_precond_sigma'
    cases = [(lambda: lib.irs_precond_workspace(*grid, 0, None), 'irs_precond_workspace: null pointer'),
             (lambda: lib.irs_precond_workspace(*grid, 3, C.byref(small)), 'irs_precond_workspace: smooth = 3, 0..2'),
             (lambda: lib.irs_precond_workspace(0, 6, 7, 0, C.byref(small)), 'irs_precond_workspace: dims (0, 6, 7), every one >= 1 needed'),
             (lambda: acc(g=None), f'{A}: null pointer'),
             (lambda: acc(v=None), f'{A}: null pointer'),
             (lambda: acc(cnt=None), f'{A}: null pointer'),
             (lambda: acc(Cn=0), f'{A}: C = 0 chains, 1..{L.IRS_MAX_CHAINS}'),
             (lambda: acc(Cn=L.IRS_MAX_CHAINS + 1), f'{A}: C = {L.IRS_MAX_CHAINS + 1} chains, 1..{L.IRS_MAX_CHAINS}'),
             (lambda: acc(d=(5, 0, 7)), f'{A}: dims (5, 0, 7), every one >= 1 needed'),
             (lambda: acc(d=(1024, 1024, 1024)), f'{A}: the volume must have fewer than 2^30 voxels'),
             (lambda: acc(beta=1.0), f'{A}: beta = 1, a value in [0, 1) needed'),
             (lambda: acc(beta=-0.5), f'{A}: beta = -0.5, a value in [0, 1) needed'),
             (lambda: acc(beta=float('nan')), f'{A}: beta = nan, a value in [0, 1) needed'),
             (lambda: acc(v=grad[1:]), f'{A}: V overlaps grad_v'),
             (lambda: acc(v=sg[:1]), f'{A}: V overlaps sigma'),
             (lambda: sig(v=None), f'{G}: null pointer'),
             (lambda: sig(o=None), f'{G}: null pointer'),
             (lambda: sig(sm=None), f'{G}: null pointer'),
             (lambda: sig(w=None), f'{G}: null pointer'),
             (lambda: sig(Cn=0), f'{G}: C = 0 chains, 1..{L.IRS_MAX_CHAINS}'),
             (lambda: sig(d=(5, 6, -1)), f'{G}: dims (5, 6, -1), every one >= 1 needed'),
             (lambda: sig(bias=0.5), f'{G}: bias = 0.5, a finite value >= 1 needed (1 / (1 - beta^t))'),
             (lambda: sig(bias=float('inf')), f'{G}: bias = inf, a finite value >= 1 needed (1 / (1 - beta^t))'),
             (lambda: sig(r=3), f'{G}: smooth = 3, 0..2'),
             (lambda: sig(r=-1), f'{G}: smooth = -1, 0..2'),
             (lambda: sig(damping=0.0), f'{G}: damping = 0, a finite value > 0 needed'),
             (lambda: sig(damping=float('inf')), f'{G}: damping = inf, a finite value > 0 needed'),
             (lambda: sig(lo=0.0), f'{G}: sigma_min = 0, sigma_max = 4, 0 < sigma_min <= 1 <= sigma_max < inf needed'),
             (lambda: sig(lo=1.5), f'{G}: sigma_min = 1.5, sigma_max = 4, 0 < sigma_min <= 1 <= sigma_max < inf needed'),
             (lambda: sig(hi=0.5), f'{G}: sigma_min = 0.25, sigma_max = 0.5, 0 < sigma_min <= 1 <= sigma_max < inf needed'),
             (lambda: sig(hi=float('inf')), f'{G}: sigma_min = 0.25, sigma_max = inf, 0 < sigma_min <= 1 <= sigma_max < inf needed'),
             (lambda: sig(wb=nbytes.value - 1), f'{G}: workspace of {nbytes.value - 1} bytes, {nbytes.value} needed (irs_precond_workspace)'),
             (lambda: sig(o=grad, v=grad[1:]), f'{G}: sigma overlaps V')]
    for call, message in cases:
        assert call() != 0 and lib.irs_last_error().decode() == message, (lib.irs_last_error().decode(), message)
    torch.cuda.synchronize()
    assert (V == 7.0).all() and (out == 7.0).all() and (summary == 7.0).all() and int(count) == 0  # nothing was launched
    assert acc() == 0 and acc(s=None) == 0 and sig() == 0 and sig(cnt=None) == 0 and sig(r=0, wb=small.value) == 0
    torch.cuda.synchronize()
    assert not (V == 7.0).any() and torch.isfinite(out).all() and float(summary[7]) == 0.0
    # the wrappers refuse shapes that do not fit the state
    state = P.preconditioner_state(grid, DEV)
    with pytest.raises(L.IrsError, match='grad_v must have shape'):
        P.preconditioner_accumulate(torch.zeros(2, 3, 5, 6, 8, device=DEV), None, state, 0.9)
    with pytest.raises(L.IrsError, match='sigma must have the shape of grad_v'):
        P.preconditioner_accumulate(grad, sg[:1], state, 0.9)
    with pytest.raises(L.IrsError, match='operators run on the GPU only'):
        P.preconditioner_accumulate(grad.cpu(), None, state, 0.9)
    assert state['count'] == 0


# ---------------------------------------------------------------- the trainer
SSD = 'synthetic_ssd_l2_128.json'
N = 24
# (a clamp tighter than the default: the test is about the plumbing, and a 24^3 chain at this learning rate should not fold)
OPTION = {'beta': 0.9, 'refresh': 4, 'until': 8, 'damping': 0.1, 'smooth': 1, 'sigma_min': 0.5, 'sigma_max': 2.0}
RUN = dict(no_chains=2, no_iters_burn_in=12, no_samples_MCMC=4, log_period_MCMC=2, checkpoint_period=3)


def make_trainer(tmp_path, option, svffd=False, **trainer_over):
    from ir_sgmcmc_amd.parse_config import ConfigParser
    from ir_sgmcmc_amd.trainer import Trainer
    cfg = json.load(open(os.path.join(ROOT, 'configs', SSD)))
    cfg['trainer']['save_dir'] = str(tmp_path)
    cfg['data_loader']['args']['dims'] = [N, N, N]
    if svffd:
        cfg['transformation_module'] = {'type': 'SVFFD_3D', 'args': {'cps': [4, 4, 4]}}
    cfg['trainer'].update(VI=False, MCMC=True, no_iters_VI=0, no_samples_VI_test=0, **{**RUN, **trainer_over})
    if option is not None:
        cfg['trainer']['adaptive_preconditioner'] = option
    config = ConfigParser.from_dict(copy.deepcopy(cfg), timestamp='t')
    dl = config.init_data_loader()
    tm, rm = config.init_transformation_and_registration_modules()
    return Trainer(config, dl, config.init_losses(), tm, rm, config.init_metrics(), device=DEV), dl


def checkpoint(t, sample_no):
    return torch.load(t.config.save_dirs['checkpoints'] / f'checkpoint_{sample_no:07}.pt', map_location='cpu', weights_only=True)


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    """one run with the option and one without, every third transition checkpointed; which transitions asked for grad_v"""
    asked = []
    plain = TransitionEngine.transition

    def spy(self, fixed, moving, v, sigma=None, eps=None, unif=None, outputs=None, timed=False):
        asked.append((outputs or {}).get('grad_v') is not None)
        return plain(self, fixed, moving, v, sigma, eps, unif, outputs, timed)

    on, _ = make_trainer(tmp_path_factory.mktemp('on'), OPTION)
    TransitionEngine.transition = spy
    try:
        on.run()
    finally:
        TransitionEngine.transition = plain
    off, _ = make_trainer(tmp_path_factory.mktemp('off'), None)
    off.run()
    return on, off, asked


def test_trainer_is_the_plain_chain_until_the_first_refresh(runs):
    on, off, _ = runs
    a, b = checkpoint(on, 3), checkpoint(off, 3)
    assert torch.equal(bits(a['v_curr_state']), bits(b['v_curr_state'])) and a['sigma'] is None and b['sigma'] is None
    assert 'preconditioner' in a and 'preconditioner' not in b and set(a) - set(b) == {'preconditioner'}
    assert a['preconditioner']['count'] == 3 and a['preconditioner']['frozen'] == -1
    assert not torch.equal(checkpoint(on, 6)['v_curr_state'], checkpoint(off, 6)['v_curr_state'])  # sigma took effect
    assert off.precond_options is None and off.preconditioner_summary is None and off._sigma is None
    assert not [k for k in off.metrics.result() if 'precond' in k]


def test_trainer_sigma_is_the_restatement_of_a_bare_engine(runs, tmp_path):
    """the first refresh, after transition 4, against the gradients of four transitions driven by hand on a second engine of
    the same configuration and seed"""
    on, _, _ = runs
    t, dl = make_trainer(tmp_path, None)
    fixed, moving, vp = next(iter(dl))
    fixed, moving = {k: v.to(DEV) for k, v in fixed.items()}, {k: v.to(DEV) for k, v in moving.items()}
    t._engine_init(fixed, moving)
    t._GMM_init(fixed, moving, vp)
    t._SGLD_init(vp)
    grad, V = torch.empty_like(t.v_curr_state), np.zeros((1, 3, N, N, N), f32)
    for _ in range(4):
        t.engine.transition(t._fixed, t._moving, t.v_curr_state, None, None, None, {**t._outputs, 'grad_v': grad})
        t.engine.flush()
        V, bad = S.accumulate(V, grad.cpu().numpy(), None, OPTION['beta'])
        assert bad == 0
    first = on.preconditioner_summary['refreshes'][0]
    assert first['step'] == 4
    bias, n = S.bias_correction(OPTION['beta'], 4), V.size
    sbar, _ = S.means(V, bias, 1, 0.1)
    _, gbar = S.means(V, bias, 1, 0.1, sbar=first['s_mean'])
    assert abs(first['s_mean'] - sbar) <= n * 2.0 ** -52 * sbar and abs(first['G_mean'] - gbar) <= n * 2.0 ** -52 * gbar
    want, summary = S.sigma_field(V, 2, bias, 1, 0.1, 0.5, 2.0, sbar=first['s_mean'], gbar=first['G_mean'])
    ck = checkpoint(on, 6)  # taken before the second refresh: it holds the field of the first
    assert ck['sigma'].numpy().tobytes() == want.tobytes()
    assert float(ck['sigma'].min()) < 1.0 < float(ck['sigma'].max())
    for key in ('sigma_min', 'sigma_max', 'clamped_low', 'clamped_high'):
        assert first[key] == summary[key]


def test_trainer_freezes_sigma_at_until(runs):
    on, _, asked = runs
    n_total = RUN['no_iters_burn_in'] + RUN['no_samples_MCMC']
    assert asked[:8] == [True] * 8 and not any(asked[8:]) and len(asked) == n_total + 100  # the speed test included
    frozen = checkpoint(on, 9)['sigma']
    assert not torch.equal(frozen, checkpoint(on, 6)['sigma'])  # the refresh at 8 changed it
    for sample_no in (12, 15):
        assert torch.equal(bits(checkpoint(on, sample_no)['sigma']), bits(frozen))
    assert torch.equal(bits(on._sigma.cpu()), bits(frozen))
    assert torch.equal(bits(on._sigma[1]), bits(on._sigma[0]))
    last = checkpoint(on, 15)['preconditioner']
    assert last['count'] == 8 and last['frozen'] == 8 and last['nonfinite'] == 0
    assert torch.equal(bits(last['V']), bits(checkpoint(on, 9)['preconditioner']['V']))


def test_trainer_resumes_bit_for_bit(runs, tmp_path):
    on, off, _ = runs
    ck = on.config.save_dirs['checkpoints'] / 'checkpoint_0000006.pt'
    b, _ = make_trainer(tmp_path / 'b', OPTION, resume=str(ck))
    b.run()
    assert torch.equal(bits(b.v_curr_state), bits(on.v_curr_state)) and torch.equal(bits(b._sigma), bits(on._sigma))
    assert torch.equal(bits(b._precond['V']), bits(on._precond['V'])) and b._precond['count'] == on._precond['count'] == 8
    assert [r['step'] for r in b.preconditioner_summary['refreshes']] == [8] and b.preconditioner_summary['frozen_at'] == 8
    # a checkpoint written without the option: refused while sigma is still adapted, taken once it is frozen
    c, _ = make_trainer(tmp_path / 'c', OPTION, resume=str(off.config.save_dirs['checkpoints'] / 'checkpoint_0000006.pt'))
    with pytest.raises(ValueError, match='the checkpoint at sample 6 holds no preconditioner state'):
        c.run()
    d, _ = make_trainer(tmp_path / 'd', OPTION, resume=str(off.config.save_dirs['checkpoints'] / 'checkpoint_0000009.pt'))
    d.run()
    assert d._sigma is None and d.preconditioner_summary['frozen_at'] == 8 and d.preconditioner_summary['refreshes'] == []
    assert torch.equal(bits(d.v_curr_state), bits(off.v_curr_state))


def test_trainer_summary_metrics_and_files(runs, tmp_path):
    on, _, _ = runs
    s = on.preconditioner_summary
    assert s['options'] == {**OPTION, 'save': True} == on.precond_options and s['frozen_at'] == 8
    assert [r['step'] for r in s['refreshes']] == [4, 8]
    for r in s['refreshes']:
        assert set(r) == {'step', *P.SUMMARY_KEYS} and r['nonfinite'] == 0
        assert 0.5 <= r['sigma_min'] < 1.0 < r['sigma_max'] <= 2.0 and r['s_mean'] > 0 and r['G_mean'] > 0
    result = on.metrics.result()
    for key in ('sigma_min', 'sigma_max', 'sigma2_mean', 'clamped_low', 'clamped_high'):
        assert f'MCMC/precond/{key}' in result
    assert result['MCMC/precond/sigma_max'] == (s['refreshes'][0]['sigma_max'] + s['refreshes'][1]['sigma_max']) / 2
    samples = on.config.save_dirs['samples']
    from ir_sgmcmc_amd.utils.imageio import read_nifti
    plain, masked = (read_nifti(str(samples / f'MCMC_precond_sigma{suffix}.nii.gz'))[0] for suffix in ('', '_masked'))
    rms = on._sigma[0].square().mean(dim=0).sqrt().cpu().numpy()
    assert plain.shape == (N, N, N) and np.array_equal(np.sort(plain, None), np.sort(rms, None)) and (masked[masked != 0] == plain[masked != 0]).all()
    # SVFFD_3D: the field lives on the control grid -- the chain runs, no file is written
    ffd, _ = make_trainer(tmp_path / 'ffd', OPTION, svffd=True)
    ffd.run()
    assert ffd._sigma.shape == ffd.v_curr_state.shape and ffd._sigma.shape[2:] != (N, N, N)
    assert [r['step'] for r in ffd.preconditioner_summary['refreshes']] == [4, 8]
    assert not list(ffd.config.save_dirs['samples'].glob('MCMC_precond_sigma*'))
    # "save": false writes nothing either
    quiet, _ = make_trainer(tmp_path / 'quiet', {**OPTION, 'save': False})
    quiet.run()
    assert not list(quiet.config.save_dirs['samples'].glob('MCMC_precond_sigma*'))
    assert torch.equal(bits(quiet._sigma), bits(on._sigma))


def test_trainer_refuses_at_construction(tmp_path):
    with pytest.raises(ValueError, match='trainer.MCMC_init = "VI" is not supported'):
        make_trainer(tmp_path / 'a', OPTION, MCMC_init='VI')
    with pytest.raises(ValueError, match=r'until must be in 1 \.\. no_iters_burn_in = 12'):
        make_trainer(tmp_path / 'b', {**OPTION, 'until': 13})
    with pytest.raises(ValueError, match='no_iters_burn_in = 0'):
        make_trainer(tmp_path / 'c', {'refresh': 4}, no_iters_burn_in=0)


def test_a_diverged_chain_raises_with_the_step(tmp_path):
    """a gradient buffer of NaN in place of transition 4's: the refresh stops the run, its message names the step, and sigma is
    left as it was"""
    t, dl = make_trainer(tmp_path, OPTION)
    fixed, moving, vp = next(iter(dl))
    fixed, moving = {k: v.to(DEV) for k, v in fixed.items()}, {k: v.to(DEV) for k, v in moving.items()}
    t._engine_init(fixed, moving)
    t._GMM_init(fixed, moving, vp)
    t._SGLD_init(vp)
    t._precond_init()
    t._precond_grad = torch.full_like(t.v_curr_state, float('nan'))
    with pytest.raises(RuntimeError, match=r'adaptive preconditioner: \d+ non-finite gradient values up to transition 4'):
        t._adapt_preconditioner(4, fixed['mask'][0], torch.ones(3))
    assert t._sigma is None
