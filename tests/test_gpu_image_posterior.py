"""Image posterior on the device (image_posterior.image_posterior_update / _finalize, diagnostics.ImagePosterior,
utils.calc_image_posterior, the trainer option) against `ops.warp`, the float64 references of tests/_exact_cases.py and the numpy
restatement of tests/_image_posterior.py.

The sample is held to `ops.warp` bit for bit (same expressions) and, on the dyadic cases, to the float64 reference exactly.
The fold: low / high are exact; the float32 Welford mean of K records stays within 5 K 2^-24 max|x| of their float64 mean
(tests/test_gpu_local_similarity.py: the recorder bound, scaled by the image's magnitude); the variance m2 / (K - 1) stays within
4 x VAR_BAND max|x|^2 of the two-pass float64 variance, VAR_BAND being what the float32 recurrence itself loses on the same
record sets (tests/test_image_posterior_host.py::test_restatement_band) -- the factor is there for the device's contraction of
m2 + d * (x - mean) into one FMA.  The finalize: range is one subtraction (bit-equal), std one division and one square root
(2 x 2^-23 relative), z five roundings of the stored maps (2^-21 relative); integer columns exact, double columns within 1e-6
relative of numpy sums over the device's stored maps.

A NaN in a source voxel: the kernel's product 0 * NaN is NaN, as in `ops.warp`, so a tap that reads the voxel with weight 0
carries it too.  The test plants the NaN where no tap reads it with weight 0 (asserted first), so "read with a non-zero weight"
and "read" name the same output voxels, and holds the device to that set and to `ops.warp` of the same volume.

Measured maxima are recorded through tests/_report.check and stated in DESIGN.md section 6."""
import copy
import ctypes as C
import json
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from ir_sgmcmc_amd import _lib as L
from ir_sgmcmc_amd import image_posterior as IP
from ir_sgmcmc_amd import ops
from ir_sgmcmc_amd.diagnostics import ImagePosterior
from tests import _exact_cases as X
from tests import _image_posterior as R
from tests._report import check

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = IP.STATE_KEYS


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def run_steps(volumes, steps, state=None, records=0):
    """fold `steps` (a list of (C,3,D,H,W) arrays) into a state -> (state, records)"""
    v = dev(volumes)
    state = IP.image_posterior_state(v.shape[0], v.shape[2:], DEV) if state is None else state
    for t in steps:
        IP.image_posterior_update(v, dev(t), state, records)
        records += t.shape[0]
    return state, records


def warps(volumes, t):
    """the device's own ops.warp of every volume -> (S,C,D,H,W)"""
    return torch.stack([ops.warp(dev(volumes[s:s + 1]), dev(t))[:, 0] for s in range(volumes.shape[0])])


# ---------------------------------------------------------------- 1. the sampler is ops.warp
@pytest.mark.parametrize('shape', [(2, 3, 5), (5, 9, 129), (33, 5, 65)])
def test_one_record_is_ops_warp_bit_for_bit(shape):
    t = R.random_transformation(shape, 1, 100 + shape[0])
    vol = R.random_volumes(shape, 1, 200 + shape[0])
    state, _ = run_steps(vol, [t])
    want = ops.warp(dev(vol), dev(t))[:, 0]
    for key in ('mean', 'low', 'high'):
        assert same_bits(state[key], want), key
    assert not state['m2'].any()
    # positions reach 3 voxels past every face
    for raw, n in zip(X.voxel_coordinates(torch.from_numpy(t), shape), X.axis_sizes(shape)):
        assert float(raw.min()) < -2.99 and float(raw.max()) > n + 1.99


# ---------------------------------------------------------------- 2. exact cases
@pytest.mark.parametrize('S', [1, 4, 5, 8])
@pytest.mark.parametrize('dims', X.EXACT_DIMS)
def test_exact_cases_hold_the_extremes_of_the_float64_reference(dims, S):
    case = X.warp_case(dims, False)
    assert case.C == 3
    g = torch.Generator().manual_seed(4000 + X.EXACT_DIMS.index(tuple(dims)))
    vols = torch.randint(0, 256, (8, 1, *dims), generator=g).float()[:S]
    assert S < 5 or not torch.equal(vols[3], vols[4])  # a group boundary cannot hide a stride error
    t = (X.identity(dims) + case.d_last).contiguous()
    state, n = run_steps(vols.numpy(), [t.numpy()])
    assert n == 3
    for s in range(S):
        ref = X.warp_reference(SimpleNamespace(**{**vars(case), 'im': vols[s:s + 1]}), torch.float64)[0][:, 0]
        assert torch.equal(state['low'][s].cpu().double(), ref.min(0).values), (s, 'low')
        assert torch.equal(state['high'][s].cpu().double(), ref.max(0).values), (s, 'high')
        # integer images on the quarter-voxel lattice: the samples are multiples of 1/64 below 256 and the mean of three is one
        # rounding of an exact sum away
        assert float((state['mean'][s].cpu().double() - ref.mean(0)).abs().max()) <= R.mean_bound(3, 255.0)


# ---------------------------------------------------------------- 3. several steps
@pytest.mark.parametrize('C_', R.STEP_CHAINS)
@pytest.mark.parametrize('shape', R.STEP_SHAPES)
def test_several_steps_against_the_devices_own_warps(shape, C_):
    volumes, steps = R.step_case(shape, C_)
    state, n = None, 0
    records = []
    for step, t in enumerate(steps):
        state, n = run_steps(volumes, [t], state, n)
        records.append(warps(volumes, t))
        rec = torch.cat(records, 1)  # (S,K,D,H,W)
        K = rec.shape[1]
        assert K == n == C_ * (step + 1)
        assert same_bits(state['low'], rec.min(1).values) and same_bits(state['high'], rec.max(1).values)
        for s in range(volumes.shape[0]):
            r = rec[s].cpu().numpy()
            magnitude = float(np.abs(r).max())
            m64, v64, _, _ = R.two_pass(r)
            mean = state['mean'][s].cpu().numpy().astype(np.float64)
            var = state['m2'][s].cpu().numpy().astype(np.float64) / max(K - 1, 1)
            frac = np.abs(mean - m64) / R.mean_bound(K, magnitude)
            err = np.abs(var - v64) / magnitude ** 2
            print(f'{shape} C={C_} K={K} volume {s}: mean {frac.max():.4f} of the bound, variance {err.max():.3e} max|x|^2 '
                  f'({err.max() / R.VAR_BAND:.3f} of the band)')
            check('image_posterior_steps', 'mean (fraction of 5 K 2^-24 max|x|)', frac, np.zeros_like(frac), 1.0)
            check('image_posterior_steps', 'variance (units of max|x|^2)', err, np.zeros_like(err), 4 * R.VAR_BAND)


# ---------------------------------------------------------------- 4. state handling
def test_state_handling_is_deterministic_and_resumable():
    shape = (5, 9, 33)
    volumes = R.random_volumes(shape, 5, 31)
    steps = [R.random_transformation(shape, 2, 40 + s) for s in range(5)]
    whole, n = run_steps(volumes, steps)
    again, _ = run_steps(volumes, steps)
    assert n == 10 and all(same_bits(whole[k], again[k]) for k in KEYS)
    # records_before = 0 overwrites whatever the state held
    junk = {k: torch.full_like(whole[k], math.nan if i % 2 else -3e30) for i, k in enumerate(KEYS)}
    junk['low'][:, ::2] = math.inf
    over, _ = run_steps(volumes, steps, junk, 0)
    assert all(same_bits(whole[k], over[k]) for k in KEYS)
    # 3 + 2 steps across a state_dict are the 5 steps
    names = [f'v{i}' for i in range(5)]
    first = ImagePosterior(dev(volumes), names, DEV)
    for t in steps[:3]:
        first.record(dev(t))
    sd = {k: (v.clone() if torch.is_tensor(v) else copy.deepcopy(v)) for k, v in first.state_dict().items()}
    assert sd['records'] == 6 and sd['names'] == names and all(sd[k].dtype == torch.float32 and not sd[k].is_cuda for k in KEYS)
    second = ImagePosterior(dev(volumes), names, DEV)
    second.load_state_dict(sd)
    for t in steps[3:]:
        second.record(dev(t))
    assert second.records == 10 and all(same_bits(whole[k], second.state[k]) for k in KEYS)
    with pytest.raises(ValueError, match='does not match'):
        ImagePosterior(dev(volumes), names[::-1], DEV).load_state_dict(sd)
    # finalize twice: identical bytes
    mask = dev(np.random.default_rng(5).random(shape) < 0.6)
    ref = dev(R.random_volumes(shape, 1, 32)[0, 0])
    a = IP.image_posterior_finalize(whole, 4, n, ref, 0.25, mask)
    b = IP.image_posterior_finalize(whole, 4, n, ref, 0.25, mask)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    out = second.finalize(mask, {'v4': ref}, 0.25)
    assert list(out) == names and 'z' in out['v4'] and 'z' not in out['v0'] and same_bits(out['v4']['std'], a[0])
    assert out['v4']['summary']['records'] == 10 and 'z_rms' in out['v4']['summary'] and 'z_rms' not in out['v0']['summary']
    # the functional form folds the same records
    from ir_sgmcmc_amd.utils import calc_image_posterior
    fn = calc_image_posterior(dev(volumes), dev(np.concatenate(steps)), {4: ref}, mask, 0.25)
    assert len(fn) == 5 and same_bits(fn[4]['z'], a[2]) and same_bits(fn[0]['mean'], whole['mean'][0])
    assert json.dumps(fn[4]['summary'], sort_keys=True) == json.dumps(out['v4']['summary'], sort_keys=True)


# ---------------------------------------------------------------- 5. non-finite input
def test_a_nan_source_voxel_poisons_exactly_its_readers():
    shape = (9, 12, 20)
    volumes = R.random_volumes(shape, 2, 51)
    planted = (4 * 12 + 6) * 20 + 9  # interior, every index >= 2: no border-clamped tap reads it with weight 0
    volumes[1].reshape(-1)[planted] = np.nan
    steps = [R.random_transformation(shape, 2, 60 + s) for s in range(2)]
    state, n, poisoned = None, 0, np.zeros(shape, bool)
    for t in steps:
        tp = R.taps(t, shape)
        weighted, read = R.readers(tp, planted, True), R.readers(tp, planted, False)
        assert np.array_equal(weighted, read) and weighted.any()  # the reference's own precondition
        poisoned |= weighted.any(0)
        state, n = run_steps(volumes, [t], state, n)
        assert np.array_equal(np.isnan(state['mean'][1].cpu().numpy()), poisoned)  # and stays poisoned
        assert np.array_equal(np.isnan(warps(volumes[1:], t)[0].cpu().numpy()), weighted)  # ops.warp of the same volume
    assert 0 < poisoned.sum() < poisoned.size and not state['mean'][0].isnan().any()
    mask = np.random.default_rng(7).random(shape) < 0.7
    mask.reshape(-1)[np.flatnonzero(poisoned)[:2]] = (True, False)  # a poisoned voxel inside the mask and one outside
    ref = R.random_volumes(shape, 1, 52)[0, 0]
    std, rng, z, isum, fsum = IP.image_posterior_finalize(state, 1, n, dev(ref), 0.1, dev(mask))
    for m in (std, rng, z):
        assert np.array_equal(np.isnan(m.cpu().numpy()), poisoned)
    ints, floats = R.summary_np(state['mean'][1].cpu().numpy(), std.cpu().numpy(), rng.cpu().numpy(), z.cpu().numpy(), mask)
    assert isum.tolist() == ints and ints[0] == int(mask.sum()) and ints[1] == int((mask & poisoned).sum()) > 0
    assert np.isfinite(fsum.cpu().numpy()).all() and np.allclose(fsum.cpu().numpy(), floats, rtol=1e-6, atol=0)
    # an empty mask: nothing enters
    _, _, _, isum0, fsum0 = IP.image_posterior_finalize(state, 1, n, dev(ref), 0.1, dev(np.zeros(shape, bool)))
    assert isum0.tolist() == [0, 0, 0, 0] and fsum0.tolist() == [0.0, 0.0, -math.inf, -math.inf, 0.0, -math.inf]
    ip = ImagePosterior(dev(volumes), ('moving', 'dose'), DEV)
    ip.load_state_dict({'records': n, 'names': ['moving', 'dose'], 'dims': list(shape), **{k: state[k].cpu() for k in KEYS}})
    s0 = ip.finalize(dev(np.zeros(shape, bool)), {'dose': dev(ref)}, 0.1)['dose']['summary']
    assert s0['voxels'] == 0 and all(math.isnan(s0[k]) for k in ('mean', 'std_mean', 'std_max', 'range_max', 'z_rms', 'z_max',
                                                                 'z_gt2', 'z_gt3'))
    s1 = ip.finalize(dev(mask), {'dose': dev(ref)}, 0.1)['dose']
    assert s1['summary']['nonfinite_voxels'] == ints[1] and np.array_equal(np.isnan(s1['mean'].cpu().numpy()), poisoned)


# ---------------------------------------------------------------- 6. the summary
@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('shape', [(41, 40, 41), (65, 64, 65)])
def test_finalize_maps_and_summary(shape, masked):
    volumes = R.random_volumes(shape, 1, 71)
    steps = [R.random_transformation(shape, 3, 80 + s) for s in range(2)]
    state, n = run_steps(volumes, steps)
    mask = (np.random.default_rng(9).random(shape) < 0.5) if masked else None
    dmask = None if mask is None else dev(mask)
    floor = 0.3
    host = {k: state[k][0].cpu().numpy() for k in KEYS}
    # without a reference: std and range against the restatement, the z columns NaN / 0
    std, rng, z, isum, fsum = IP.image_posterior_finalize(state, 0, n, None, floor, dmask)
    assert z is None
    std_np, rng_np, _ = R.finalize_np(*(host[k] for k in KEYS), n)
    assert np.array_equal(rng.cpu().numpy(), rng_np)
    assert (np.abs(std.cpu().numpy().astype(np.float64) - std_np) <= 2.0 ** -22 * std_np).all()
    ints, floats = R.summary_np(host['mean'], std.cpu().numpy(), rng.cpu().numpy(), None, mask)
    assert isum.tolist() == ints and ints[2:] == [0, 0] and ints[0] == (int(mask.sum()) if masked else int(np.prod(shape)))
    got = fsum.cpu().numpy()
    assert np.isnan(got[4:]).all() and np.allclose(got[:4], floats[:4], rtol=1e-6, atol=0)
    # a reference none of whose |z| lies within 1e-4 of a threshold: draw one, then move the voxels that come close
    ref = R.random_volumes(shape, 1, 72)[0, 0]
    spread = np.sqrt(std.cpu().numpy().astype(np.float64) ** 2 + float(np.float32(floor)) ** 2)
    z0 = np.abs(R.z_np(host['mean'], std.cpu().numpy(), ref, floor))
    near = (np.abs(z0 - 2) < 1e-3) | (np.abs(z0 - 3) < 1e-3)
    ref = np.where(near, ref + 0.01 * spread, ref).astype(np.float32)
    z_ref = R.z_np(host['mean'], std.cpu().numpy(), ref, floor)
    assert not (np.abs(np.abs(z_ref) - 2) < 1e-4).any() and not (np.abs(np.abs(z_ref) - 3) < 1e-4).any()
    std2, rng2, z, isum, fsum = IP.image_posterior_finalize(state, 0, n, dev(ref), floor, dmask)
    assert same_bits(std2, std) and same_bits(rng2, rng)
    zd = z.cpu().numpy().astype(np.float64)
    rel = np.abs(zd - z_ref) / np.maximum(np.abs(z_ref), 1e-30)
    check('image_posterior_finalize', 'z (relative)', rel, np.zeros_like(rel), 2.0 ** -21)
    ints, floats = R.summary_np(host['mean'], std.cpu().numpy(), rng.cpu().numpy(), zd, mask)
    inside = np.ones(shape, bool) if mask is None else mask
    assert ints[2] == int((np.abs(z_ref)[inside] > 2).sum()) > ints[3] == int((np.abs(z_ref)[inside] > 3).sum()) > 0
    assert isum.tolist() == ints
    assert np.allclose(fsum.cpu().numpy(), floats, rtol=1e-6, atol=0), (fsum.tolist(), floats)


# ---------------------------------------------------------------- 7. refusals
def test_refusals_return_errors_and_nothing_faults():
    lib = L.load()
    buf = torch.zeros(1 << 16, device=DEV)
    p = C.c_void_p(buf.data_ptr())
    for fn, good, cases in R.abi_refusals(p):
        for cid, replaced, msg in cases:
            rc, err = R.abi_call(lib, fn, good, replaced)
            assert rc != 0 and err == f'{fn}: {msg}', (fn, cid, rc, err)
    shape = (4, 5, 6)
    volumes, t = dev(R.random_volumes(shape, 2, 1)), dev(R.random_transformation(shape, 2, 2))
    state = IP.image_posterior_state(2, shape, DEV)
    for kw, msg in ((dict(records_before=-1), 'records_before = -1'), (dict(records_before=2 ** 31 - 2), 'overflow'),
                    (dict(volumes=volumes[:, :, :, :, :5].contiguous()), 'does not match'), (dict(volumes=volumes[:, 0]), 'does not match'),
                    (dict(volumes=volumes.double()), 'float32'), (dict(transformation=t[:, :2].contiguous()), 'expected a'),
                    (dict(transformation=t.cpu()), 'GPU only'), (dict(volumes=volumes.repeat(5, 1, 1, 1, 1)), '1 .. 8'),
                    (dict(state={**state, 'high': state['high'][:1]}), 'high must be')):
        with pytest.raises(L.IrsError, match=msg):
            IP.image_posterior_update(**{'volumes': volumes, 'transformation': t, 'state': state, 'records_before': 0, **kw})
    IP.image_posterior_update(volumes, t, state, 0)
    ref = torch.zeros(shape, device=DEV)
    for kw, msg in ((dict(n=0), 'n = 0'), (dict(index=2), 'index'), (dict(std_floor=-0.5), 'std_floor'),
                    (dict(std_floor=math.nan), 'std_floor'), (dict(reference=ref[:, :, :5]), 'reference must be'),
                    (dict(reference=ref.double()), 'reference must be'), (dict(mask=torch.ones(4, 5, device=DEV, dtype=torch.bool)), 'mask must be'),
                    (dict(mask=torch.ones(shape, device=DEV)), 'mask must be')):
        with pytest.raises(L.IrsError, match=msg):
            IP.image_posterior_finalize(**{'state': state, 'index': 0, 'n': 2, **kw})
    with pytest.raises(ValueError, match='reference for'):
        ip = ImagePosterior(volumes, ('moving', 'dose'), DEV)
        ip.record(t)
        ip.finalize(None, {'pet': ref})
    with pytest.raises(ValueError, match='S, 1, 4, 5, 6'):
        from ir_sgmcmc_amd.utils import calc_image_posterior
        calc_image_posterior(volumes[:, 0], t)
    # and the device is as it was: the same call as before the refusals, the same bits
    again = IP.image_posterior_state(2, shape, DEV)
    IP.image_posterior_update(volumes, t, again, 0)
    torch.cuda.synchronize()
    assert all(same_bits(state[k], again[k]) for k in KEYS)


# ---------------------------------------------------------------- 8. the trainer
def make_trainer(tmp_path, dims, **trainer_over):
    from ir_sgmcmc_amd.parse_config import ConfigParser
    from ir_sgmcmc_amd.trainer import Trainer
    cfg = json.load(open(os.path.join(ROOT, 'configs', 'synthetic_gmm_lognormal.json')))
    cfg['trainer']['save_dir'] = str(tmp_path)
    cfg['data_loader']['args']['dims'] = list(dims)
    cfg['trainer'].update(trainer_over)
    config = ConfigParser.from_dict(copy.deepcopy(cfg), timestamp='t')
    dl = config.init_data_loader()
    losses = config.init_losses()
    tm, rm = config.init_transformation_and_registration_modules()
    return Trainer(config, dl, losses, tm, rm, config.init_metrics(), device=DEV)


def test_trainer_image_posterior(tmp_path, monkeypatch):
    from ir_sgmcmc_amd.diagnostics import image_posterior_metric_names, recorded_steps
    from ir_sgmcmc_amd.utils.imageio import read_nifti, write_nifti
    N = 24
    ramp = np.broadcast_to(np.arange(N, dtype=np.float32), (N, N, N)).copy()  # f = x index
    path = str(tmp_path / 'ramp.nii.gz')
    write_nifti(ramp, path)
    kw = dict(no_chains=2, no_iters_burn_in=2, no_samples_MCMC=8, log_period_MCMC=4, checkpoint_period=6)
    on_kw = dict(kw, image_posterior={'period': 1, 'volumes': [{'name': 'ramp', 'path': path}]})
    seen = []  # the transformations the recorder took, step by step
    update = ImagePosterior._update
    monkeypatch.setattr(ImagePosterior, '_update', lambda self, t: (seen.append(t.detach().cpu().clone()), update(self, t))[1])
    torch.manual_seed(0)
    a = make_trainer(tmp_path / 'a', (N, N, N), **on_kw)
    a.run()
    monkeypatch.setattr(ImagePosterior, '_update', update)
    C_ = a.no_chains
    res = a.metrics.result()
    new = image_posterior_metric_names(a.image_options)
    assert len(new) == 3 + 3 + 3 and all(a.metrics._count[k] > 0 and not math.isnan(res[k]) for k in new)
    s = a.image_summary
    assert list(s) == ['moving', 'ramp'] and set(s['moving']) == set(s['ramp']) | {'z_rms', 'z_max', 'z_gt2', 'z_gt3'}
    fixed, moving, _ = next(iter(a.data_loader))
    mask = (fixed['mask'].reshape(N, N, N) != 0).numpy()
    for name in s:
        for key in ('std_mean', 'std_max', 'range_max'):
            assert res[f'MCMC/image/{name}/{key}'] == s[name][key]
        assert s[name]['voxels'] == int(mask.sum()) and s[name]['nonfinite_voxels'] == 0
        assert 0 <= s[name]['std_mean'] <= s[name]['std_max'] <= s[name]['range_max']
    for key in ('z_rms', 'z_gt2', 'z_gt3'):
        assert res[f'MCMC/image/moving/{key}'] == s['moving'][key]
    assert 0 <= s['moving']['z_gt3'] <= s['moving']['z_gt2'] <= 1 and s['moving']['z_rms'] <= s['moving']['z_max']
    assert s['moving']['records'] == C_ * len(recorded_steps(2, 8, 1)) == a._image_posterior.records == C_ * len(seen) == 16
    # the floor of z: 1e-3 of the moving image's intensity range
    lo, hi = float(moving['im'].min()), float(moving['im'].max())
    assert a._image_std_floor == pytest.approx(1e-3 * (hi - lo), rel=1e-6)
    assert same_bits(a._image_volumes[0], moving['im'][0].to(DEV)) and same_bits(a._image_volumes[1, 0], dev(ramp))
    # the ramp reads the x position: where no record leaves the volume along x, mean_ramp - x is the mean x displacement of the
    # same records in voxels, and std_ramp its std
    t_all = torch.cat(seen).double()  # (records,3,N,N,N)
    pos = (t_all[:, 0] + 1.0) / 2.0 * (N - 1)
    inside = ((pos >= 0) & (pos <= N - 1)).all(0).numpy()
    assert inside.mean() > 0.5
    disp = (pos - torch.arange(N, dtype=torch.float64)).numpy()
    maps = a.image_maps['ramp']
    d_mean = np.abs(maps['mean'].cpu().numpy().astype(np.float64) - ramp - disp.mean(0))[inside]
    d_std = np.abs(maps['std'].cpu().numpy().astype(np.float64) - disp.std(0, ddof=1))[inside]
    print(f'ramp: mean x displacement off by {d_mean.max():.3e}, its std by {d_std.max():.3e} voxels; largest |displacement| '
          f'{np.abs(disp).max():.3f}, largest std {disp.std(0, ddof=1).max():.3f}')
    check('image_posterior_trainer', 'ramp mean - x against the mean x displacement (voxels)', d_mean, np.zeros_like(d_mean), 1e-4)
    check('image_posterior_trainer', 'ramp std against the std of the x displacement (voxels)', d_std, np.zeros_like(d_std), 1e-4)
    assert np.abs(disp).max() > 0.05 and disp.std(0, ddof=1).max() > 1e-3  # the chain moved
    # the files hold the maps, NaN as 0, the masked ones 0 outside the fixed mask
    folder = a.config.save_dirs['samples']
    new_files = [f'MCMC_im_{name}_{key}{tail}.nii.gz' for name in ('moving', 'ramp') for key in ('mean', 'std', 'range')
                 for tail in ('', '_masked')] + ['MCMC_im_moving_z.nii.gz', 'MCMC_im_moving_z_masked.nii.gz']
    for name, volume in a.image_maps.items():
        assert set(volume) == {'mean', 'std', 'range', 'summary'} | ({'z'} if name == 'moving' else set())
        for key in ('mean', 'std', 'range', 'z'):
            if key in volume:
                im = torch.nan_to_num(volume[key].cpu(), nan=0.0).numpy()
                plain, _ = read_nifti(str(folder / f'MCMC_im_{name}_{key}.nii.gz'))
                masked, _ = read_nifti(str(folder / f'MCMC_im_{name}_{key}_masked.nii.gz'))
                assert (plain == im).all() and (masked[mask] == im[mask]).all() and not masked[~mask].any()
    # resumed from the checkpoint in the middle of the recording, the state and the summary come out bit for bit
    ck = a.config.save_dirs['checkpoints'] / 'checkpoint_0000006.pt'
    sd = torch.load(ck, map_location='cpu', weights_only=True)
    assert sd['image_posterior']['records'] == C_ * 4 and sd['image_posterior']['names'] == ['moving', 'ramp']
    assert tuple(sd['image_posterior']['mean'].shape) == (2, N, N, N)
    torch.manual_seed(0)
    b = make_trainer(tmp_path / 'b', (N, N, N), resume=str(ck), **on_kw)
    b.run()
    assert all(same_bits(a._image_posterior.state[k], b._image_posterior.state[k]) for k in KEYS)
    assert json.dumps(a.image_summary, sort_keys=True) == json.dumps(b.image_summary, sort_keys=True)
    assert same_bits(a.v_curr_state, b.v_curr_state)
    del sd['image_posterior']
    torch.save(sd, tmp_path / 'no_image.pt')
    with pytest.raises(ValueError, match='image_posterior'):
        make_trainer(tmp_path / 'c', (N, N, N), resume=str(tmp_path / 'no_image.pt'), **on_kw).run()
    # with the option off: the same chain, the same metric keys, files and checkpoint keys as without the feature
    torch.manual_seed(0)
    off = make_trainer(tmp_path / 'off', (N, N, N), **kw)
    off.run()
    assert same_bits(off.v_curr_state, a.v_curr_state) and same_bits(off.displacement_mean, a.displacement_mean)
    off_keys = list(off.metrics.result())
    assert not [k for k in off_keys if k.startswith('MCMC/image/')]
    assert [k for k in res if not k.startswith('MCMC/image/')] == off_keys and sorted(res) == sorted(off_keys + new)
    assert off.image_options is None and off._image_posterior is None and off._image_volumes is None and off.image_summary is None
    names = lambda tr: sorted(p.name for p in tr.config.save_dirs['samples'].iterdir())
    assert names(a) == sorted(names(off) + new_files)
    sd_off = torch.load(off.config.save_dirs['checkpoints'] / 'checkpoint_0000006.pt', map_location='cpu', weights_only=True)
    assert set(sd_off) == set(sd)


# ---------------------------------------------------------------- 9. the affine map
def test_an_extra_volume_goes_through_the_pre_alignment_of_the_moving_image(tmp_path):
    from ir_sgmcmc_amd.parse_config import ConfigParser
    from ir_sgmcmc_amd.trainer import Trainer
    from ir_sgmcmc_amd.utils.imageio import write_nifti
    N = 32
    cfg = json.load(open(os.path.join(ROOT, 'configs', 'synthetic_ssd_l2_128_affine.json')))
    cfg['trainer']['save_dir'] = str(tmp_path)
    cfg['data_loader']['args'].update(dims=[N, N, N], misalign={'rotation_deg': [4.0, 0.0, 0.0], 'shift': [0.0, 2.0, 0.0]})
    cfg['trainer'].update(no_chains=2, no_iters_burn_in=2, no_samples_MCMC=4, log_period_MCMC=2, save_outputs=False,
                          affine_init={'model': 'rigid', 'levels': [[16, 16, 16]]})
    config = ConfigParser.from_dict(copy.deepcopy(cfg), timestamp='probe', make_dirs=False)
    _, moving, _ = next(iter(config.init_data_loader()))
    path = str(tmp_path / 'copy_of_moving.nii.gz')
    write_nifti(moving['im'][0, 0].numpy(), path)  # the MISALIGNED moving image, as the loader yields it
    cfg['trainer']['image_posterior'] = {'period': 1, 'volumes': [{'name': 'copy', 'path': path}], 'save': False}
    config = ConfigParser.from_dict(copy.deepcopy(cfg), timestamp='t')
    tm, rm = config.init_transformation_and_registration_modules()
    t = Trainer(config, config.init_data_loader(), config.init_losses(), tm, rm, config.init_metrics(), device=DEV)
    t.run()
    assert t.affine_summary is not None and t.affine_summary['iterations'] >= 2
    vols = t._image_volumes
    assert same_bits(vols[0], vols[1]) and not torch.equal(vols[0, 0].cpu(), moving['im'][0, 0])  # both went through the map
    st = t._image_posterior.state
    assert t._image_posterior.records == 8 and all(same_bits(st[k][0], st[k][1]) for k in KEYS)
    assert float(st['m2'][0].max()) > 0
    s = t.image_summary
    assert {k: v for k, v in s['moving'].items() if not k.startswith('z_')} == s['copy']
