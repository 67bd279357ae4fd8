"""Split-R-hat convergence diagnostics on the device: the moment update and the finalize kernel against a float64 numpy
restatement, the masked summary against numpy on the returned map, determinism, the ABI refusals, and the trainer option
end to end (files, metrics, checkpoint / resume, and nothing at all when it is off)."""
import copy
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from ir_sgmcmc_amd import _lib as L
from ir_sgmcmc_amd import ops
from ir_sgmcmc_amd.diagnostics import ChainMoments, recorded_steps
from ir_sgmcmc_amd.parse_config import ConfigParser
from ir_sgmcmc_amd.trainer import Trainer
from ir_sgmcmc_amd.utils import calc_split_rhat
from tests._split_rhat import split_rhat_map_np

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 2e-5


def draw(C, N, shape, offset, seed):
    """(C, N, 3, *shape) float32; offset: chains drawn around different centres (and a drift between halves), so R >> 1.
    Voxel (0, 0, 0) is the same constant in every chain (W = B = 0: R = 1); component 0 of voxel (0, 0, 1) is constant
    within each sequence but differs between them (W = 0 < B: R = inf)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((C, N, 3, *shape)).astype(np.float32)
    if offset:
        x += (3.0 * np.arange(C, dtype=np.float32)).reshape(C, 1, 1, 1, 1, 1)
        x[:, N - N // 2:] += 1.5
        x *= rng.uniform(0.5, 2.0, size=(1, 1, 3, *shape)).astype(np.float32)
    x[:, :, :, 0, 0, 0] = 2.5
    x[:, :, 0, 0, 0, 1] = (np.arange(C).reshape(C, 1) + (np.arange(N) >= N // 2)).astype(np.float32)
    return x


def moments_np(x):
    """per-half, per-chain mean and M2 in float64 -> (2, C, 3, ...) each"""
    C, N = x.shape[:2]
    n = N // 2
    halves = [x[:, :n].astype(np.float64), x[:, N - n:].astype(np.float64)]
    mean = np.stack([h.mean(axis=1) for h in halves])
    m2 = np.stack([((h - h.mean(axis=1, keepdims=True)) ** 2).sum(axis=1) for h in halves])
    return mean, m2


def assert_map_close(got, ref):
    got = np.asarray(got, dtype=np.float64)
    assert not np.isnan(got).any()
    assert np.array_equal(np.isinf(got), np.isinf(ref))
    fin = np.isfinite(ref)
    rel = np.abs(got[fin] - ref[fin]) / np.abs(ref[fin])
    assert rel.max() < RTOL, rel.max()


def summary_np(rhat, mask, thresholds=(1.01, 1.1)):
    r = rhat.reshape(-1) if mask is None else rhat.reshape(-1)[mask.reshape(-1)]
    r64 = r.astype(np.float64)
    return {'voxels': r.size, 'max': float(r64.max()), 'sum': float(r64.sum()),
            'above': [int((r > np.float32(t)).sum()) for t in thresholds]}


CASES = [  # C, N, shape, offset
    (1, 8, (7, 9, 11), False),
    (1, 9, (5, 13, 6), True),
    (2, 6, (7, 9, 11), True),
    (2, 11, (9, 7, 5), False),
    (2, 4, (3, 4, 17), True),
    (3, 10, (6, 5, 9), False),
    (3, 7, (11, 3, 7), True),
]


@pytest.mark.parametrize('C,N,shape,offset', CASES)
def test_moments_and_map_match_numpy(C, N, shape, offset):
    x = draw(C, N, shape, offset, seed=C * 100 + N)
    cm = ChainMoments(C, shape, N, DEV)
    xd = torch.from_numpy(x).to(DEV)
    for i in range(N):
        cm.record(xd[:, i].contiguous())
    mean_ref, m2_ref = moments_np(x)
    n = N // 2
    assert np.allclose(cm.mean.cpu().numpy(), mean_ref, rtol=1e-5, atol=1e-5)
    assert np.allclose(cm.m2.cpu().numpy(), m2_ref, rtol=1e-5, atol=1e-5 * n)
    rhat, summary = cm.rhat()
    ref = split_rhat_map_np(x)
    assert ref[0, 0, 0] == 1.0 and np.isinf(ref[0, 0, 1])
    assert_map_close(rhat.cpu().numpy(), ref)
    if offset:
        assert summary['frac_above_1.1'] > 0.9
    else:
        assert np.median(ref) < 1.5
    # the functional form computes the same map
    rhat_f, summary_f = calc_split_rhat(xd)
    assert torch.equal(rhat_f, rhat) and summary_f == summary


@pytest.mark.parametrize('with_mask', [False, True])
@pytest.mark.parametrize('C,N,shape,offset', [CASES[2], CASES[5]])
def test_summary_matches_numpy_on_the_returned_map(C, N, shape, offset, with_mask):
    x = draw(C, N, shape, offset, seed=7)
    cm = ChainMoments(C, shape, N, DEV)
    xd = torch.from_numpy(x).to(DEV)
    for i in range(N):
        cm.record(xd[:, i].contiguous())
    mask = None
    if with_mask:
        mask = torch.from_numpy(np.random.default_rng(3).random(shape) < 0.5)
        mask[0, 0, 0] = True
    thresholds = (1.01, 1.1)
    rhat, summary = cm.rhat(mask, thresholds)
    r = rhat.cpu().numpy()
    ref = summary_np(r, None if mask is None else mask.numpy(), thresholds)
    assert summary['voxels'] == ref['voxels']
    assert summary['above_1.01'] == ref['above'][0] and summary['above_1.1'] == ref['above'][1]
    assert summary['max'] == ref['max']
    mean_ref = ref['sum'] / ref['voxels']
    if np.isinf(mean_ref):
        assert summary['mean'] == mean_ref
    else:
        assert abs(summary['mean'] - mean_ref) <= 1e-12 * abs(mean_ref)
    assert summary['frac_above_1.1'] == ref['above'][1] / ref['voxels']
    # a finite case as well: without the W = 0 < B voxel, max and mean are finite
    if mask is not None:
        mask[0, 0, 1] = False
        rhat2, s2 = cm.rhat(mask, thresholds)
        ref2 = summary_np(rhat2.cpu().numpy(), mask.numpy(), thresholds)
        assert np.isfinite(s2['max']) and s2['max'] == ref2['max']
        assert abs(s2['mean'] - ref2['sum'] / ref2['voxels']) <= 1e-12 * abs(s2['mean'])


def test_two_finalize_calls_are_bit_identical():
    C, N, shape = 2, 12, (37, 41, 43)  # more than one block of partials
    x = torch.from_numpy(draw(C, N, shape, True, seed=11)).to(DEV)
    cm = ChainMoments(C, shape, N, DEV)
    for i in range(N):
        cm.record(x[:, i].contiguous())
    mask = (torch.rand(shape, generator=torch.Generator().manual_seed(2)) < 0.3).to(DEV)
    a = ops.split_rhat(cm.mean, cm.m2, cm.n, mask)
    b = ops.split_rhat(cm.mean, cm.m2, cm.n, mask)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert a[1].dtype == torch.float64 and int(a[1][0]) == int(mask.sum())


def test_abi_refusals():
    lib = L.load()
    C_, D, H, W = 2, 5, 6, 7
    x = torch.zeros(C_, 3, D, H, W, device=DEV)
    mean = torch.zeros(2, C_, 3, D, H, W, device=DEV)
    m2 = torch.zeros_like(mean)
    rhat = torch.empty(D, H, W, device=DEV)
    summary = torch.empty(5, device=DEV, dtype=torch.float64)
    nb = C.c_size_t()
    L.check(lib.irs_split_rhat_workspace(C_, D, H, W, C.byref(nb)))
    ws = torch.empty(nb.value, device=DEV, dtype=torch.uint8)
    p = lambda t: C.c_void_p(t.data_ptr())
    st = L.stream_ptr()

    def upd(x_=x, C=C_, D=D, H=H, W=W, half=0, k=1, mean_=mean, m2_=m2):
        return lib.irs_chain_moments_update(None if x_ is None else p(x_), C, D, H, W, half, k,
                                            None if mean_ is None else p(mean_), None if m2_ is None else p(m2_), st)

    def fin(mean_=mean, m2_=m2, C=C_, n=2, rhat_=rhat, summary_=summary, ws_=ws, ws_bytes=nb.value, D=D, H=H, W=W):
        q = lambda t: None if t is None else p(t)
        return lib.irs_split_rhat(q(mean_), q(m2_), C, n, None, 1.01, 1.1, q(rhat_), q(summary_), q(ws_), ws_bytes, D, H, W, st)

    L.check(upd())
    L.check(fin())
    torch.cuda.synchronize()
    bad_update = [dict(C=0), dict(D=0), dict(H=-1), dict(W=0), dict(half=2), dict(half=-1), dict(k=0), dict(x_=None),
                  dict(mean_=None), dict(m2_=None)]
    bad_finalize = [dict(C=0), dict(D=0), dict(W=-3), dict(n=1), dict(n=0), dict(mean_=None), dict(m2_=None), dict(rhat_=None),
                    dict(summary_=None), dict(ws_=None), dict(ws_bytes=nb.value - 1)]
    for kw in bad_update:
        with pytest.raises(L.IrsError):
            L.check(upd(**kw))
    for kw in bad_finalize:
        with pytest.raises(L.IrsError):
            L.check(fin(**kw))
    with pytest.raises(L.IrsError):
        L.check(lib.irs_split_rhat_workspace(0, D, H, W, C.byref(nb)))
    # the Python surface checks shapes and dtypes before it calls
    with pytest.raises(L.IrsError):
        ops.chain_moments_update(x, mean[:1], m2[:1], 0, 1)
    with pytest.raises(L.IrsError):
        ops.chain_moments_update(x.double(), mean, m2, 0, 1)
    with pytest.raises(L.IrsError):
        ops.split_rhat(mean, m2, 2, mask=torch.ones(D, H, W + 1, device=DEV, dtype=torch.bool))
    with pytest.raises(L.IrsError):
        ops.split_rhat(mean, m2[:, :1], 2)


# ---------------------------------------------------------------- the trainer option
def make_trainer(tmp_path, name, dims, **trainer_over):
    cfg = json.load(open(os.path.join(ROOT, 'configs', name)))
    cfg['trainer']['save_dir'] = str(tmp_path)
    cfg['data_loader']['args']['dims'] = list(dims)
    cfg['trainer'].update(trainer_over)
    config = ConfigParser.from_dict(copy.deepcopy(cfg), timestamp='t')
    dl = config.init_data_loader()
    losses = config.init_losses()
    tm, rm = config.init_transformation_and_registration_modules()
    return Trainer(config, dl, losses, tm, rm, config.init_metrics(), device=DEV), dl


def test_trainer_rhat_matches_the_saved_samples(tmp_path):
    from ir_sgmcmc_amd.utils.imageio import read_nifti, read_vtk_vectors
    N = 24
    kw = dict(no_iters_burn_in=4, no_samples_MCMC=10, log_period_MCMC=2, save_samples=True, convergence_diagnostics=True)
    t, _ = make_trainer(tmp_path, 'synthetic_gmm_lognormal.json', (N, N, N), **kw)
    t.run()
    C = t.no_chains
    assert C == 2
    steps = recorded_steps(4, 10, 2)  # 6 .. 14: the saved samples too (the burn-in is a multiple of the period)
    folder = t.config.save_dirs['samples']
    samples = np.stack([np.stack([read_vtk_vectors(str(folder / 'MCMC' / f'chain_{c}_sample_{s:07}_displacement.vtk'))[2]
                                  for s in steps]) for c in range(C)])
    assert samples.shape == (C, len(steps), 3, N, N, N)
    ref = split_rhat_map_np(samples)
    got = t.rhat.cpu().numpy()
    assert got.shape == (N, N, N)
    assert_map_close(got, ref)
    im, _ = read_nifti(str(folder / 'MCMC_rhat.nii.gz'))
    assert np.array_equal(im, got)
    masked, _ = read_nifti(str(folder / 'MCMC_rhat_masked.nii.gz'))
    _, moving, _ = next(iter(t.data_loader))
    mask = moving['mask'][0].reshape(N, N, N).numpy() != 0
    assert np.array_equal(masked[mask], got[mask]) and not masked[~mask].any()
    s = t.rhat_summary
    assert s['voxels'] == int(mask.sum()) and s['max'] == float(got[mask].max())
    res = t.metrics.result()
    for key in ('max', 'mean', 'frac_above_1.01', 'frac_above_1.1'):
        assert res[f'MCMC/R_hat/{key}'] == s[key]


def test_trainer_rhat_survives_checkpoint_resume_bit_for_bit(tmp_path):
    kw = dict(no_iters_burn_in=4, no_samples_MCMC=12, log_period_MCMC=2, checkpoint_period=8,
              convergence_diagnostics={'period': 2})
    a, _ = make_trainer(tmp_path / 'a', 'synthetic_gmm_lognormal.json', (16, 16, 16), **kw)
    a.run()
    ck = a.config.save_dirs['checkpoints'] / 'checkpoint_0000008.pt'
    sd = torch.load(ck, map_location='cpu', weights_only=True)
    assert sd['chain_moments']['count'] == 2
    b, _ = make_trainer(tmp_path / 'b', 'synthetic_gmm_lognormal.json', (16, 16, 16), resume=str(ck), **kw)
    b.run()
    assert torch.equal(a.rhat, b.rhat) and a.rhat_summary == b.rhat_summary
    assert torch.equal(a.displacement_std, b.displacement_std)


def test_trainer_option_off_changes_nothing(tmp_path):
    kw = dict(no_iters_burn_in=4, no_samples_MCMC=8, log_period_MCMC=2, checkpoint_period=6)
    t, _ = make_trainer(tmp_path, 'synthetic_gmm_lognormal.json', (16, 16, 16), **kw)
    t.run()
    assert t.rhat is None and t.rhat_summary is None
    assert not [k for k in t.metrics.result() if 'R_hat' in k]
    assert not list(t.config.save_dirs['samples'].glob('*rhat*'))
    sd = torch.load(t.config.save_dirs['checkpoints'] / 'checkpoint_0000006.pt', map_location='cpu', weights_only=True)
    assert set(sd) == {'v_curr_state', 'sigma', 'tau', 'engine_state', 'sample_no', 'moments', 'config_name'}
