"""Split ESS and MCSE on the device: the variogram update and the finalize against the float64 numpy restatement, the masked
summary against numpy on the returned maps, determinism, the ABI refusals, and the trainer option end to end (files,
metrics, R-hat and std maps untouched, checkpoint / resume)."""
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
from ir_sgmcmc_amd.utils import calc_split_ess
from tests._split_ess import ess_from_stats, split_ess_map_np, var_plus_np, variogram_np

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-5


def draw(C, N, shape, seed):
    """(C, N, 3, *shape) float32 AR(1) chains, phi drawn per element over [-0.5, 0.95], a different centre per chain.
    Voxel (0, 0, 0) is the same constant everywhere (var+ = 0: ESS = mn); component 0 of voxel (0, 0, 1) is constant within
    each sequence but differs between them (S_t = 0, rho_t = 1: truncated, tau = 1 + 2T)."""
    rng = np.random.default_rng(seed)
    phi = rng.uniform(-0.5, 0.95, size=(3, *shape))
    x = np.empty((C, N, 3, *shape))
    x[:, 0] = rng.standard_normal((C, 3, *shape)) / np.sqrt(1 - phi ** 2)
    for i in range(1, N):
        x[:, i] = phi * x[:, i - 1] + rng.standard_normal((C, 3, *shape))
    x += rng.uniform(-0.2, 0.2, size=(C, 1, 1, 1, 1, 1))
    x = x.astype(np.float32)
    x[:, :, :, 0, 0, 0] = 2.5
    x[:, :, 0, 0, 0, 1] = (np.arange(C).reshape(C, 1) * 2 + (np.arange(N) >= N // 2)).astype(np.float32)
    return x


def record_all(x, max_lag):
    C, N = x.shape[:2]
    cm = ChainMoments(C, x.shape[3:], N, DEV, max_lag=max_lag)
    xd = torch.from_numpy(x).to(DEV)
    for i in range(N):
        cm.record(xd[:, i].contiguous())
    return cm, xd


def reference_from_device_sums(x, cm):
    """the restatement fed the device's own lag sums: (ess, mcse, truncated, margin) maps"""
    C, N = x.shape[:2]
    ess, mcse, tr, margin = ess_from_stats(var_plus_np(x), cm.vsum.double().cpu().numpy(), 2 * C, N // 2, cm.max_lag)
    return ess.min(axis=0), mcse.max(axis=0), tr.any(axis=0), margin.min(axis=0)


def assert_close(got, ref, keep=None, rtol=RTOL):
    got = np.asarray(got, dtype=np.float64)
    assert not np.isnan(got).any()
    keep = np.ones(ref.shape, dtype=bool) if keep is None else keep
    assert np.array_equal(np.isinf(got)[keep], np.isinf(ref)[keep])
    fin = keep & np.isfinite(ref)
    err = np.abs(got[fin] - ref[fin])
    assert (err <= rtol * np.abs(ref[fin])).all(), (err / np.maximum(np.abs(ref[fin]), 1e-300)).max()


CASES = [  # C, N, shape, max_lag: L below / above n - 1, odd / even N, C * 3 * V a multiple of 4 or not
    (1, 12, (7, 9, 11), 3),
    (1, 13, (4, 6, 5), 8),
    (2, 16, (4, 6, 5), 4),
    (2, 11, (7, 9, 11), 32),
    (2, 40, (3, 5, 7), 8),
    (3, 20, (6, 5, 9), 5),
    (3, 9, (4, 4, 4), 6),
]


@pytest.mark.parametrize('C,N,shape,max_lag', CASES)
def test_variogram_matches_numpy(C, N, shape, max_lag):
    x = draw(C, N, shape, seed=C * 100 + N)
    cm, _ = record_all(x, max_lag)
    ref = variogram_np(x, max_lag)
    got = cm.vsum.double().cpu().numpy()
    assert got.shape == ref.shape
    assert (np.abs(got - ref) <= RTOL * ref).all(), np.abs(got - ref).max()
    # the ring holds the last min(n, L) samples of half 1 in their slots
    n = N // 2
    for k in range(max(1, n - max_lag + 1), n + 1):
        assert torch.equal(cm.ring[(k - 1) % max_lag].cpu(), torch.from_numpy(x[:, N - n + k - 1]))


@pytest.mark.parametrize('C,N,shape,max_lag', CASES)
def test_ess_matches_the_restatement(C, N, shape, max_lag):
    x = draw(C, N, shape, seed=C * 100 + N)
    cm, xd = record_all(x, max_lag)
    ess, mcse, summary = cm.ess()
    ess, mcse = ess.cpu().numpy(), mcse.cpu().numpy()
    n, mn = N // 2, 2 * C * (N // 2)
    # the finalize fed the device's own lag sums (only a decision on a knife edge, |rho_{T+1} + rho_{T+2}| < 1e-6, could
    # differ with var+ taken from the fp32 moments)
    e_ref, s_ref, tr_ref, margin = reference_from_device_sums(x, cm)
    keep = margin >= 1e-6
    assert keep.mean() > 0.99
    assert_close(ess, e_ref, keep)
    assert_close(mcse, s_ref, keep)
    # the degenerate voxels
    assert ess[0, 0, 0] == mn and mcse[0, 0, 0] == 0.0
    Lp = min(max_lag, n - 1)
    T = Lp if Lp % 2 else Lp - 1
    assert tr_ref[0, 0, 1] and ess[0, 0, 1] == pytest.approx(mn / (1 + 2 * T), rel=RTOL)
    if keep.all():
        assert summary['truncated'] == int(tr_ref.sum())
    # end to end from the samples, excluding the components whose truncation decision is within 1e-3 of flipping
    e2, s2, _, margin2 = split_ess_map_np(x, max_lag)
    keep2 = margin2 >= 1e-3
    assert keep2.mean() > 0.8
    assert_close(ess, e2, keep2)
    assert_close(mcse, s2, keep2)
    assert not np.isnan(ess).any() and not np.isnan(mcse).any() and (ess > 0).all()
    # the functional form computes the same maps
    ess_f, mcse_f, summary_f = calc_split_ess(xd, max_lag=max_lag)
    assert np.array_equal(ess_f.cpu().numpy(), ess) and np.array_equal(mcse_f.cpu().numpy(), mcse) and summary_f == summary


def test_non_finite_samples_give_zero_and_inf():
    C, N, shape = 2, 10, (4, 5, 6)
    x = draw(C, N, shape, seed=5)
    x[1, 2, 1, 3, 3, 3] = np.inf
    cm, _ = record_all(x, 4)
    ess, mcse, _ = cm.ess()
    assert ess[3, 3, 3] == 0 and mcse[3, 3, 3] == float('inf')
    assert not torch.isnan(ess).any() and not torch.isnan(mcse).any()


@pytest.mark.parametrize('with_mask', [False, True])
@pytest.mark.parametrize('C,N,shape,max_lag', [CASES[2], CASES[5]])
def test_summary_matches_numpy_on_the_returned_maps(C, N, shape, max_lag, with_mask):
    x = draw(C, N, shape, seed=7)
    cm, _ = record_all(x, max_lag)
    mask = None
    if with_mask:
        mask = torch.from_numpy(np.random.default_rng(3).random(shape) < 0.5)
        mask[0, 0, 0] = mask[0, 0, 1] = True
    thr = 20.0
    ess, mcse, summary = cm.ess(mask, thr)
    e = ess.cpu().numpy().reshape(-1)
    sel = np.ones(e.shape, dtype=bool) if mask is None else mask.numpy().reshape(-1)
    e = e[sel]
    _, _, tr_ref, margin = reference_from_device_sums(x, cm)
    assert margin.min() >= 1e-6
    assert summary['voxels'] == e.size
    assert summary[f'below_{thr:g}'] == int((e < np.float32(thr)).sum())
    assert summary['truncated'] == int(tr_ref.reshape(-1)[sel].sum())
    assert summary['min'] == float(e.min())
    mean_ref = e.astype(np.float64).sum() / e.size
    assert abs(summary['mean'] - mean_ref) <= 1e-12 * mean_ref
    assert summary[f'frac_below_{thr:g}'] == summary[f'below_{thr:g}'] / e.size
    assert summary['frac_truncated'] == summary['truncated'] / e.size
    # an empty mask: no voxels, NaN statistics rather than a division by zero
    if with_mask:
        _, _, s0 = cm.ess(torch.zeros(shape, dtype=torch.bool), thr)
        assert s0['voxels'] == 0 and s0['truncated'] == 0 and np.isnan(s0['min']) and np.isnan(s0['mean'])


def test_two_update_sequences_and_two_finalize_calls_are_bit_identical():
    C, N, shape, max_lag = 2, 14, (37, 41, 43), 5  # more than one block of partials
    x = draw(C, N, shape, seed=11)
    a, _ = record_all(x, max_lag)
    b, _ = record_all(x, max_lag)
    assert torch.equal(a.ring, b.ring) and torch.equal(a.vsum, b.vsum)
    mask = (torch.rand(shape, generator=torch.Generator().manual_seed(2)) < 0.3).to(DEV)
    r1 = ops.split_ess(a.mean, a.m2, a.vsum, a.n, mask)
    r2 = ops.split_ess(a.mean, a.m2, a.vsum, a.n, mask)
    for u, v in zip(r1, r2):
        assert torch.equal(u, v)
    assert r1[2].dtype == torch.float64 and int(r1[2][0]) == int(mask.sum())


def test_abi_refusals():
    lib = L.load()
    C_, D, H, W, Lg = 2, 5, 6, 7, 4
    x = torch.zeros(C_, 3, D, H, W, device=DEV)
    ring = torch.zeros(Lg, C_, 3, D, H, W, device=DEV)
    vsum = torch.zeros(Lg, 3, D, H, W, device=DEV)
    mean = torch.zeros(2, C_, 3, D, H, W, device=DEV)
    m2 = torch.zeros_like(mean)
    ess = torch.empty(D, H, W, device=DEV)
    mcse = torch.empty(D, H, W, device=DEV)
    summary = torch.empty(5, device=DEV, dtype=torch.float64)
    nb = C.c_size_t()
    L.check(lib.irs_split_ess_workspace(C_, D, H, W, C.byref(nb)))
    ws = torch.empty(nb.value, device=DEV, dtype=torch.uint8)
    q = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    st = L.stream_ptr()

    def upd(x_=x, C=C_, D=D, H=H, W=W, k=1, L_=Lg, ring_=ring, vsum_=vsum):
        return lib.irs_chain_variogram_update(q(x_), C, D, H, W, k, L_, q(ring_), q(vsum_), st)

    def fin(mean_=mean, m2_=m2, vsum_=vsum, C=C_, n=4, L_=Lg, ess_=ess, mcse_=mcse, summary_=summary, ws_=ws,
            ws_bytes=nb.value, D=D, H=H, W=W):
        return lib.irs_split_ess(q(mean_), q(m2_), q(vsum_), C, n, L_, None, 400.0, q(ess_), q(mcse_), q(summary_), q(ws_),
                                 ws_bytes, D, H, W, st)

    L.check(upd())
    L.check(fin())
    torch.cuda.synchronize()
    bad_update = [dict(C=0), dict(C=9), dict(D=0), dict(H=-1), dict(W=1), dict(k=0), dict(k=-3), dict(L_=0), dict(x_=None),
                  dict(ring_=None), dict(vsum_=None)]
    bad_finalize = [dict(C=0), dict(D=0), dict(W=-3), dict(n=3), dict(n=1), dict(L_=0), dict(mean_=None), dict(m2_=None),
                    dict(vsum_=None), dict(ess_=None), dict(mcse_=None), dict(summary_=None), dict(ws_=None),
                    dict(ws_bytes=nb.value - 1)]
    for kw in bad_update:
        with pytest.raises(L.IrsError):
            L.check(upd(**kw))
    for kw in bad_finalize:
        with pytest.raises(L.IrsError):
            L.check(fin(**kw))
    # the Python surface checks shapes, dtypes and the device before it calls
    with pytest.raises(L.IrsError):
        ops.chain_variogram_update(x, ring[:, :1], vsum, 1)
    with pytest.raises(L.IrsError):
        ops.chain_variogram_update(x, ring, vsum[:2], 1)
    with pytest.raises(L.IrsError):
        ops.chain_variogram_update(x.double(), ring, vsum, 1)
    with pytest.raises(L.IrsError):
        ops.chain_variogram_update(x.cpu(), ring, vsum, 1)
    with pytest.raises(L.IrsError):
        ops.split_ess(mean, m2, vsum[:, :2], 4)
    with pytest.raises(L.IrsError):
        ops.split_ess(mean, m2, vsum, 4, mask=torch.ones(D, H, W + 1, device=DEV, dtype=torch.bool))
    with pytest.raises(L.IrsError):
        ops.split_ess(mean, m2, vsum, 3)


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


def test_trainer_ess_matches_the_saved_samples(tmp_path):
    from ir_sgmcmc_amd.utils.imageio import read_nifti, read_vtk_vectors
    N = 24
    kw = dict(no_iters_burn_in=4, no_samples_MCMC=16, log_period_MCMC=1, save_samples=True)
    torch.manual_seed(0)  # the starting velocity is drawn from the global generator: the same for both runs below
    t, _ = make_trainer(tmp_path / 'ess', 'synthetic_gmm_lognormal.json', (N, N, N),
                        convergence_diagnostics={'period': 1, 'ess': {'max_lag': 4}}, **kw)
    t.run()
    C = t.no_chains
    steps = recorded_steps(4, 16, 1)  # 5 .. 20: every saved sample
    folder = t.config.save_dirs['samples']
    samples = np.stack([np.stack([read_vtk_vectors(str(folder / 'MCMC' / f'chain_{c}_sample_{s:07}_displacement.vtk'))[2]
                                  for s in steps]) for c in range(C)])
    assert samples.shape == (C, len(steps), 3, N, N, N)
    got_e, got_s = t.ess.cpu().numpy(), t.mcse.cpu().numpy()
    assert got_e.shape == got_s.shape == (N, N, N)
    ess_f, mcse_f, _ = calc_split_ess(torch.from_numpy(samples.astype(np.float32)).to(DEV), max_lag=4)
    assert_close(got_e, ess_f.double().cpu().numpy())
    assert_close(got_s, mcse_f.double().cpu().numpy())
    e_ref, s_ref, _, margin = split_ess_map_np(samples, 4)
    keep = margin >= 1e-3
    assert keep.mean() > 0.8
    assert_close(got_e, e_ref, keep, rtol=1e-4)
    # files, metrics, summary
    _, moving, _ = next(iter(t.data_loader))
    mask = moving['mask'][0].reshape(N, N, N).numpy() != 0
    for name, got in (('ess', got_e), ('mcse', got_s)):
        im, _ = read_nifti(str(folder / f'MCMC_{name}.nii.gz'))
        assert np.array_equal(im, got)
        masked, _ = read_nifti(str(folder / f'MCMC_{name}_masked.nii.gz'))
        assert np.array_equal(masked[mask], got[mask]) and not masked[~mask].any()
    s = t.ess_summary
    assert s['voxels'] == int(mask.sum()) and s['min'] == float(got_e[mask].min())
    res = t.metrics.result()
    for key in ('min', 'mean', 'frac_below_400', 'frac_truncated'):
        assert res[f'MCMC/ESS/{key}'] == s[key]
    # the same run with ESS off: bit-identical R-hat and std maps, and no ESS anything
    torch.manual_seed(0)
    off, _ = make_trainer(tmp_path / 'off', 'synthetic_gmm_lognormal.json', (N, N, N),
                          convergence_diagnostics={'period': 1}, **kw)
    off.run()
    assert torch.equal(off.rhat, t.rhat) and off.rhat_summary == t.rhat_summary
    assert torch.equal(off.displacement_std, t.displacement_std) and torch.equal(off.displacement_mean, t.displacement_mean)
    assert off.ess is None and off.mcse is None and off.ess_summary is None
    assert not [k for k in off.metrics.result() if 'ESS' in k]
    assert not list(off.config.save_dirs['samples'].glob('*ess*')) and not list(off.config.save_dirs['samples'].glob('*mcse*'))


def test_trainer_ess_survives_checkpoint_resume_bit_for_bit(tmp_path):
    kw = dict(no_iters_burn_in=4, no_samples_MCMC=16, log_period_MCMC=2, checkpoint_period=8,
              convergence_diagnostics={'period': 2, 'ess': {'max_lag': 3}})
    a, _ = make_trainer(tmp_path / 'a', 'synthetic_gmm_lognormal.json', (16, 16, 16), **kw)
    a.run()
    ck = a.config.save_dirs['checkpoints'] / 'checkpoint_0000008.pt'
    sd = torch.load(ck, map_location='cpu', weights_only=True)
    cm = sd['chain_moments']
    assert cm['count'] == 2 and cm['max_lag'] == 3 and tuple(cm['ring'].shape) == (3, 2, 3, 16, 16, 16)
    b, _ = make_trainer(tmp_path / 'b', 'synthetic_gmm_lognormal.json', (16, 16, 16), resume=str(ck), **kw)
    b.run()
    assert torch.equal(a.ess, b.ess) and torch.equal(a.mcse, b.mcse) and a.ess_summary == b.ess_summary
    assert torch.equal(a.rhat, b.rhat)
    # a checkpoint without the variogram, once a recorded step has passed, is refused
    for key in ('ring', 'vsum', 'max_lag'):
        del cm[key]
    ck2 = tmp_path / 'no_variogram.pt'
    torch.save(sd, ck2)
    c, _ = make_trainer(tmp_path / 'c', 'synthetic_gmm_lognormal.json', (16, 16, 16), resume=str(ck2), **kw)
    with pytest.raises(ValueError, match='max_lag'):
        c.run()
