"""Local similarity maps on the device (ops.local_similarity, local_similarity_update / _finalize, diagnostics.LocalSimilarity,
the trainer option) against the float64 numpy restatement of tests/_local_similarity.py.

The map bounds.  Write e = n 2^-52 (n the window size), E_xx = S_xx / n, R_x = E_xx / var_x.  A sum of n non-negative float64
terms, each exact, carries at most (n - 1) 2^-53 of its value in rounding, whatever the order: |d mu_x| <= (e / 2) sqrt(E_xx),
|d E_xx| <= (e / 2) E_xx, so to first order |d var_x| <= 1.5 e E_xx and |d cov| <= (e / 2) E|fm| + |mu_f d mu_m| +
|mu_m d mu_f| <= 1.5 e sqrt(E_ff E_mm).
  LNCC = cov / sqrt(var_f var_m), |LNCC| <= 1: the variances move it by at most 0.75 e (R_f + R_m), the covariance by
  1.5 e sqrt(R_f R_m) <= 0.75 e (R_f + R_m); the clamp moves nothing apart.  One evaluation: 1.5 e (R_f + R_m); the device and
  the restatement, each in its own order: 3 e (R_f + R_m), held to 4 e (R_f + R_m), plus the one rounding of the stored
  float32, 2^-24 |ref|, held to 2^-23 |ref| (rounding the reference alone reaches 0.86 of the tighter form).
  SSIM = (A1 / B1)(A2 / B2) with A1 = 2 mu_f mu_m + c1 <= B1 = mu_f^2 + mu_m^2 + c1 and |A2| = |2 cov + c2| <= B2 = var_f +
  var_m + c2.  With T = E_ff + E_mm: |d A1|, |d B1| <= e T, |d A2| <= 3 e sqrt(E_ff E_mm) <= 1.5 e T, |d B2| <= 1.5 e T, so
  one evaluation moves SSIM by at most 2 e T / B1 + 3 e T / B2 and two by 4 e T (1 / B1 + 1.5 / B2): the same construction
  with SSIM's two denominators, plus 2^-23 |ref|.
The inputs keep every window variance above 2.8e-3 against floors of 1e-6, so no voxel is near the flatness threshold.

The recorder bound.  mean_k = mean_{k-1} + (x - mean_{k-1}) / k in float32 with |x| <= 1: the difference (<= 2), the quotient
(<= 2 / k) and the sum (<= 1) round by at most u (2 + 2 / k + 1) <= 5 u together, u = 2^-24, and an earlier error enters the
next mean with the factor 1 - 1 / k <= 1: after K samples at most 5 K u.

Measured maxima (fraction of the bound) are recorded through tests/_report.check and stated in DESIGN.md section 6."""
import copy
import json
import math
import os

import numpy as np
import pytest
import torch

from ir_sgmcmc_amd import _lib as L
from ir_sgmcmc_amd import ops
from tests import _local_similarity as S
from tests._report import check

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = S.UNIT
CONSTS = ops.local_similarity_constants(UNIT, UNIT)
COL = {k: j for j, k in enumerate(S.COLUMNS)}

# a volume smaller than the window on every axis, ragged tiles, several tiles in x and in y, a z extent many windows long
SHAPES = [(1, 1, 3), (2, 3, 5), (5, 7, 9), (4, 8, 16), (17, 16, 65), (70, 9, 5), (3, 37, 70)]
RADII = [1, 2, 4]
CHAINS = [(1, 1), (2, 1), (2, 2), (3, 1), (3, 3)]  # (C, Cf)
MASKS = [None, 'bool', 'uint8']


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def gpu(fixed, moving, mask=None, radius=2, fr=UNIT, mr=UNIT, want=('lncc', 'ssim')):
    out = ops.local_similarity(dev(fixed), dev(moving), None if mask is None else dev(mask)[None, None], radius, fr, mr, want)
    return {k: v.cpu().numpy() for k, v in out.items()}


def bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


def compare_maps(name, got, refs):
    """got: the device dict of C chains; refs: one reference_maps per chain.  NaN positions equal, elsewhere within the bound;
    -> the largest fraction of the bound used, (lncc, ssim)"""
    worst = [0.0, 0.0]
    for c, ref in enumerate(refs):
        for j, (key, bound) in enumerate((('lncc', S.lncc_bound(ref)), ('ssim', S.ssim_bound(ref)))):
            g, r = got[key][c, 0].astype(np.float64), ref[key]
            assert got[key].dtype == np.float32 and g.shape == r.shape
            assert (np.isnan(g) == np.isnan(r)).all(), (name, key, c, int(np.isnan(g).sum()), int(np.isnan(r).sum()))
            ok = ~np.isnan(r)
            if ok.any():
                frac = np.abs(g[ok] - r[ok]) / bound[ok]
                worst[j] = max(worst[j], float(frac.max()))
    print(f'{name}: LNCC error {worst[0]:.3f} of its bound, SSIM error {worst[1]:.3f} of its bound')
    check('local_similarity', 'lncc_fraction_of_bound', worst[0], 0.0, 1.0)
    check('local_similarity', 'ssim_fraction_of_bound', worst[1], 0.0, 1.0)
    return worst


def compare_stats(name, got, refs, mask):
    """counts equal, NaN where the restatement has NaN, +inf where it has +inf, the float statistics to 1e-9 absolute"""
    want = np.array([[S.reference_stats(ref, mask)[k] for k in S.COLUMNS] for ref in refs], dtype=np.float64)
    g = got['stats']
    assert g.dtype == np.float64 and g.shape == want.shape
    assert (g[:, :3] == want[:, :3]).all(), (name, g[:, :3], want[:, :3])
    assert (np.isnan(g) == np.isnan(want)).all() and (np.isinf(g) == np.isinf(want)).all(), (name, g, want)
    for k in S.COLUMNS[3:]:
        ok = np.isfinite(want[:, COL[k]])
        check('local_similarity', k, g[ok, COL[k]], want[ok, COL[k]], 1e-9)
    return want


@pytest.mark.parametrize('r', RADII)
@pytest.mark.parametrize('shape', SHAPES)
def test_against_the_restatement(shape, r):
    """every (C, Cf) and mask kind at this shape and radius; the references of the chains are computed once"""
    # the seeds are chosen so that no window is near flat: the three voxels of (1, 1, 3) can fall close together
    fixed, moving = S.noise_pair(shape, 3, seed=13 + sum(shape) + r)
    shared = [S.reference_maps(fixed[0, 0], moving[c, 0], r, CONSTS) for c in range(3)]
    own = [shared[0]] + [S.reference_maps(fixed[c, 0], moving[c, 0], r, CONSTS) for c in (1, 2)]
    for ref in shared + own:
        assert ref['finite'].all() and not ref['flat'].any()
        assert min(ref['var_f'].min(), ref['var_m'].min()) >= 2.8e-3
    for C, Cf in CHAINS:
        refs = (shared if Cf == 1 else own)[:C]
        for kind in MASKS:
            mask = None if kind is None else S.random_mask(shape, sum(shape) + C, bool if kind == 'bool' else np.uint8)
            name = f'{shape} r={r} C={C} Cf={Cf} mask={kind}'
            got = gpu(fixed[:Cf], moving[:C], mask, r)
            assert got['lncc'].shape == got['ssim'].shape == (C, 1) + tuple(shape) and got['stats'].shape == (C, L.IRS_LOCAL_STATS)
            compare_maps(name, got, refs)
            want = compare_stats(name, got, refs, mask)
            assert (want[:, COL['n_flat']] == 0).all() and (want[:, COL['n_nonfinite']] == 0).all()
            assert (want[:, COL['n']] == (np.prod(shape) if mask is None else int((mask != 0).sum()))).all()


@pytest.mark.parametrize('shape,r', [((5, 7, 9), 1), ((17, 16, 65), 2), ((70, 9, 5), 4), ((3, 37, 70), 4)])
def test_unambiguous_flat_regions(shape, r):
    """half the volume constant 0.5, the rest drawn from {0, 1}: a window with one non-constant voxel has a variance of at
    least 0.25 (n - 1) / n^2 >= 3.4e-4, an all-constant one of 0 -- nothing is near the floors of 1e-6"""
    rng = np.random.default_rng(7 + r)
    vols = []
    for axis in (0, 2):
        v = rng.integers(0, 2, (1, 1) + shape).astype(np.float32)
        half = [slice(None)] * 5
        half[2 + axis] = slice(0, max(shape[axis] // 2, 1))
        v[tuple(half)] = 0.5
        vols.append(v)
    fixed, moving = vols
    ref = S.reference_maps(fixed[0, 0], moving[0, 0], r, CONSTS)
    mask = S.random_mask(shape, 11)
    got = gpu(fixed, moving, mask, r)
    assert (np.isnan(got['lncc'][0, 0]) == ref['flat']).all() and not np.isnan(got['ssim']).any()
    compare_maps(f'flat {shape} r={r}', got, [ref])
    want = compare_stats(f'flat {shape} r={r}', got, [ref], mask)
    if min(shape) > 2 * r + 2:
        assert 0 < want[0, COL['n_flat']] < want[0, COL['n']]


@pytest.mark.parametrize('shape,r', [((17, 16, 65), 1), ((17, 16, 65), 4), ((70, 9, 5), 2), ((70, 9, 5), 4)])
def test_nonfinite_values_spoil_their_windows_only(shape, r):
    """a NaN, a +inf and a -inf at an interior, a face and a corner voxel: exactly the voxels whose clamped window holds one
    are NaN in both maps, every other voxel -- the planes after the window has left the bad voxel along z among them -- is
    within the bound"""
    D, H, W = shape
    fixed, moving = S.noise_pair(shape, 2, seed=3 + r)
    interior, face, corner = (D // 3, H // 2, W // 2), (D // 2, 0, W // 3), (D - 1, H - 1, 0)
    fixed[0, 0][interior] = np.nan
    moving[0, 0][face] = np.inf
    moving[1, 0][corner] = -np.inf
    moving[1, 0][0, 0, 0] = np.nan
    mask = S.random_mask(shape, 13, np.uint8)
    refs = [S.reference_maps(fixed[0, 0], moving[c, 0], r, CONSTS) for c in range(2)]
    # the restatement's NaN set, stated once more by index arithmetic: clamping only repeats border voxels, so the clamped window
    # of a voxel holds p exactly when the voxel is within r of p on every axis
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing='ij')
    reach = lambda p: (np.abs(z - p[0]) <= r) & (np.abs(y - p[1]) <= r) & (np.abs(x - p[2]) <= r)
    assert (~refs[0]['finite'] == (reach(interior) | reach(face))).all()
    assert (~refs[1]['finite'] == (reach(interior) | reach(corner) | reach((0, 0, 0)))).all()
    got = gpu(fixed[:1], moving, mask, r)
    for c in range(2):
        bad = ~refs[c]['finite']
        assert np.isnan(got['lncc'][c, 0][bad]).all() and np.isnan(got['ssim'][c, 0][bad]).all()
        assert not np.isnan(got['lncc'][c, 0][~bad]).any() and not np.isnan(got['ssim'][c, 0][~bad]).any()
        after = slice(interior[0] + r + 1, D)  # the planes the window reaches once it has left the NaN along z
        assert not np.isnan(got['ssim'][c, 0][after][~bad[after]]).any() and (~bad[after]).any()
    compare_maps(f'nonfinite {shape} r={r}', got, refs)
    want = compare_stats(f'nonfinite {shape} r={r}', got, refs, mask)
    assert (want[:, COL['n_nonfinite']] > 0).all()


def test_repeats_and_batching_are_bit_identical():
    """two identical calls; chain c of a batch against the single-chain call, with odd voxel counts so that the bases of the
    chains are unaligned"""
    for shape, r in (((5, 7, 9), 2), ((17, 15, 65), 4), ((3, 37, 71), 1)):
        fixed, moving = S.noise_pair(shape, 3, seed=21)
        moving[1, 0][tuple(s // 2 for s in shape)] = np.nan
        mask = S.random_mask(shape, 22)
        for Cf in (1, 3):
            a, b = gpu(fixed[:Cf], moving, mask, r), gpu(fixed[:Cf], moving, mask, r)
            for key in ('lncc', 'ssim', 'stats'):
                assert (bits(a[key]) == bits(b[key])).all(), (shape, r, key)
            for c in range(3):
                one = gpu(fixed[c:c + 1] if Cf == 3 else fixed[:1], moving[c:c + 1], mask, r)
                for key in ('lncc', 'ssim', 'stats'):
                    assert (bits(one[key][0]) == bits(a[key][c])).all(), (shape, r, Cf, c, key)
        only = gpu(fixed[:1], moving, mask, r, want=())
        assert set(only) == {'stats'} and (bits(only['stats']) == bits(gpu(fixed[:1], moving, mask, r)['stats'])).all()


def test_ranges_default_to_those_of_the_images():
    fixed, moving = S.noise_pair((6, 7, 8), 2, seed=31)
    fixed, moving = (3.0 * fixed[:1] - 1.0).astype(np.float32), (0.5 * moving).astype(np.float32)
    fr, mr = (float(fixed.min()), float(fixed.max())), (float(moving.min()), float(moving.max()))
    a = ops.local_similarity(dev(fixed), dev(moving))
    b = ops.local_similarity(dev(fixed), dev(moving), None, 2, fr, mr)
    for key in ('lncc', 'ssim', 'stats'):
        assert torch.equal(a[key].view(torch.int32), b[key].view(torch.int32))
    refs = [S.reference_maps(fixed[0, 0], moving[c, 0], 2, ops.local_similarity_constants(fr, mr)) for c in range(2)]
    got = {k: v.cpu().numpy() for k, v in a.items()}
    compare_maps('ranges', got, refs)
    compare_stats('ranges', got, refs, None)


def test_refusals():
    f = torch.zeros(2, 1, 4, 5, 6, device=DEV)
    for kw in (dict(radius=0), dict(radius=5), dict(radius=2.0), dict(want=('ncc',)), dict(fixed_range=(1.0, 1.0)),
               dict(mask=torch.ones(4, 5, 6, dtype=torch.bool, device=DEV)), dict(mask=torch.ones(1, 1, 4, 5, 6, device=DEV))):
        with pytest.raises(L.IrsError):
            ops.local_similarity(f[:1], f, **{'fixed_range': UNIT, 'moving_range': UNIT, **kw})
    with pytest.raises(L.IrsError):
        ops.local_similarity(f[:, :, :3], f, fixed_range=UNIT, moving_range=UNIT)
    state = lambda: (torch.zeros(4, 5, 6, device=DEV), torch.zeros(4, 5, 6, device=DEV), torch.zeros(4, 5, 6, dtype=torch.int32, device=DEV))
    mean, low, count = state()
    for bad in ((mean[:3], low, count), (mean, low.double(), count), (mean, low, count.long())):
        with pytest.raises(L.IrsError):
            ops.local_similarity_update(f, *bad, 0)
        with pytest.raises(L.IrsError):
            ops.local_similarity_finalize(*bad)
    with pytest.raises(L.IrsError, match='records_before'):
        ops.local_similarity_update(f, mean, low, count, -1)


# ---------------------------------------------------------------- the recorder
def recorder_inputs(shape, steps=5, C=2, seed=41):
    """LNCC-like maps in [-1, 1]; voxel (0,0,1) is NaN in some records, voxel (0,0,2) in all of them"""
    rng = np.random.default_rng(seed)
    maps = (2.0 * rng.random((steps, C, 1) + shape) - 1.0).astype(np.float32)
    maps[1, 0, 0, 0, 0, 1] = maps[3, 1, 0, 0, 0, 1] = maps[4, 0, 0, 0, 0, 1] = np.nan
    maps[:, :, 0, 0, 0, 2] = np.nan
    return maps


def test_the_recorder_against_a_two_pass_reference():
    from ir_sgmcmc_amd.diagnostics import LocalSimilarity
    shape = (5, 7, 9)
    maps = recorder_inputs(shape)
    K = maps.shape[0] * maps.shape[1]
    flat = maps.reshape((K,) + shape).astype(np.float64)
    count = (~np.isnan(flat)).sum(0)
    with np.errstate(invalid='ignore', divide='ignore'):
        mean = np.where(count > 0, np.nansum(flat, 0) / count, np.nan)
    low = np.where(count > 0, np.nanmin(np.where(np.isnan(flat), np.inf, flat), 0), np.nan)
    assert count[0, 0, 1] == K - 3 and count[0, 0, 2] == 0 and (count.ravel()[3:] == K).all()
    mask = S.random_mask(shape, 42)
    mask[0, 0, :3] = True
    bound = 5 * K * 2.0 ** -24

    whole, first = LocalSimilarity(shape, DEV), LocalSimilarity(shape, DEV)
    for step in maps:
        whole.record(dev(step))
    assert whole.records == K and (whole.count.cpu().numpy() == count).all()
    g_mean, g_low, s = whole.finalize(dev(mask))
    g_mean, g_low = g_mean.cpu().numpy(), g_low.cpu().numpy()
    assert g_mean.dtype == np.float32 and (np.isnan(g_mean) == (count == 0)).all() and (np.isnan(g_low) == (count == 0)).all()
    some = count > 0
    dev_mean = check('local_similarity', 'recorder_mean', g_mean[some], mean[some], bound)
    print(f'recorder: mean error {dev_mean:.3e}, {dev_mean / bound:.3f} of the float32 Welford bound {bound:.3e}')
    assert (g_low[some].astype(np.float64) == low[some]).all()
    # the summary against sums over the reference maps
    inside = mask & some
    assert s['records'] == K and s['voxels'] == int(mask.sum()) and s['empty_voxels'] == int((mask & ~some).sum()) == 1
    assert abs(s['lncc_mean'] - mean[inside].mean()) <= bound
    assert abs(s['lncc_mean_min'] - mean[inside].min()) <= bound and s['lncc_min'] == low[inside].min()
    # and exactly those of the device's own maps
    assert s['lncc_mean_min'] == float(g_mean[inside].min())
    assert abs(s['lncc_mean'] - g_mean[inside].astype(np.float64).mean()) <= 1e-12

    # 3 + 2 records across a state_dict: bit-identical
    for step in maps[:3]:
        first.record(dev(step))
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in first.state_dict().items()}
    assert sd['records'] == 6 and sd['count'].dtype == torch.int32 and sd['mean'].dtype == torch.float32 == sd['low'].dtype
    second = LocalSimilarity(shape, DEV)
    second.load_state_dict(sd)
    for step in maps[3:]:
        second.record(dev(step))
    for name in ('mean', 'low', 'count'):
        assert torch.equal(getattr(second, name).view(torch.int32), getattr(whole, name).view(torch.int32)), name
    assert json.dumps(second.finalize(dev(mask))[2], sort_keys=True) == json.dumps(s, sort_keys=True)
    with pytest.raises(ValueError, match='does not match'):
        LocalSimilarity((5, 7, 8), DEV).load_state_dict(sd)
    with pytest.raises(RuntimeError, match='nothing recorded'):
        LocalSimilarity(shape, DEV).finalize()
    # an empty mask: nothing enters
    s0 = whole.finalize(dev(np.zeros(shape, bool)))[2]
    assert s0['voxels'] == 0 and math.isnan(s0['lncc_mean']) and math.isnan(s0['lncc_min'])


# ---------------------------------------------------------------- the trainer
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


def test_trainer_local_similarity(tmp_path):
    from ir_sgmcmc_amd.diagnostics import local_similarity_metric_names, recorded_steps
    from ir_sgmcmc_amd.utils.imageio import read_nifti
    N = 24
    kw = dict(no_chains=2, no_iters_burn_in=2, no_samples_MCMC=8, log_period_MCMC=4, checkpoint_period=6)
    on_kw = dict(kw, local_similarity={'radius': 2, 'period': 1})
    torch.manual_seed(0)
    a = make_trainer(tmp_path / 'a', (N, N, N), **on_kw)
    a.run()
    C = a.no_chains
    res = a.metrics.result()
    new = local_similarity_metric_names(C)
    assert len(new) == 3 * (C + 2) and all(a.metrics._count[k] > 0 and not math.isnan(res[k]) for k in new)
    s = a.local_similarity_summary
    assert set(s) == {'unregistered', 'mean', 'posterior'}
    fixed, moving, _ = next(iter(a.data_loader))
    mask = fixed['mask'].reshape(N, N, N) != 0
    for name, prefix in (('unregistered', 'VI/train/local_similarity'), ('mean', 'MCMC/local_similarity_of_mean')):
        assert s[name]['n'] + s[name]['n_nonfinite'] == int(mask.sum()) and s[name]['n_nonfinite'] == 0
        assert s[name]['lncc_mean'] == res[f'{prefix}/LNCC'] and s[name]['lncc_min'] == res[f'{prefix}/LNCC_min']
        assert s[name]['ssim_mean'] == res[f'{prefix}/SSIM'] and -1.0 <= s[name]['lncc_min'] <= s[name]['lncc_mean'] <= 1.0
    # registration must improve the local agreement
    print(f"LNCC of the unregistered pair {res['VI/train/local_similarity/LNCC']:.6f}, of the posterior mean "
          f"{res['MCMC/local_similarity_of_mean/LNCC']:.6f}")
    assert res['MCMC/local_similarity_of_mean/LNCC'] > res['VI/train/local_similarity/LNCC']
    # the step-0 statistics are those of the operator on the pair itself
    vol = lambda t: t.reshape(1, 1, N, N, N).contiguous().to(DEV)
    want = ops.local_similarity(vol(fixed['im']), vol(moving['im']), vol(fixed['mask']), 2, *a._local_ranges, want=())
    assert s['unregistered']['lncc_mean'] == float(want['stats'][0, COL['lncc_mean']])
    # the posterior: every recorded step of both chains
    post = s['posterior']
    assert post['records'] == C * len(recorded_steps(2, 8, 1)) == a._local_similarity.records
    assert post['voxels'] == int(mask.sum()) and -1.0 <= post['lncc_min'] <= post['lncc_mean_min'] <= post['lncc_mean'] <= 1.0
    count = a._local_similarity.count.cpu()
    assert int(count.max()) == post['records'] and post['empty_voxels'] == int((count == 0)[mask].sum())
    folder = a.config.save_dirs['samples']
    for name, im in (('lncc_mean', a.local_lncc_mean), ('lncc_min', a.local_lncc_min)):
        im = torch.nan_to_num(im.cpu(), nan=0.0).numpy()
        plain, _ = read_nifti(str(folder / f'MCMC_{name}.nii.gz'))
        masked, _ = read_nifti(str(folder / f'MCMC_{name}_masked.nii.gz'))
        m = mask.numpy()
        assert (plain == im).all() and (masked[m] == im[m]).all() and not masked[~m].any() and not np.isnan(plain).any()
    for name in ('lncc', 'ssim'):
        vol, _ = read_nifti(str(folder / f'MCMC_{name}_of_mean.nii.gz'))
        assert vol.shape == (N, N, N) and np.isfinite(vol).all() and vol.max() <= 1.0
    # resumed from the checkpoint in the middle of the recording, the state comes out bit for bit
    ck = a.config.save_dirs['checkpoints'] / 'checkpoint_0000006.pt'
    sd = torch.load(ck, map_location='cpu', weights_only=True)
    assert sd['local_similarity']['records'] == C * 4 and tuple(sd['local_similarity']['count'].shape) == (N, N, N)
    torch.manual_seed(0)
    b = make_trainer(tmp_path / 'b', (N, N, N), resume=str(ck), **on_kw)
    b.run()
    for name in ('mean', 'low', 'count'):
        assert torch.equal(getattr(a._local_similarity, name).view(torch.int32), getattr(b._local_similarity, name).view(torch.int32))
    assert json.dumps(post, sort_keys=True) == json.dumps(b.local_similarity_summary['posterior'], sort_keys=True)
    assert torch.equal(a.v_curr_state.view(torch.int32), b.v_curr_state.view(torch.int32))
    # a checkpoint without the recorder, once a recorded step has passed, is refused
    del sd['local_similarity']
    torch.save(sd, tmp_path / 'no_local.pt')
    with pytest.raises(ValueError, match='local_similarity'):
        make_trainer(tmp_path / 'c', (N, N, N), resume=str(tmp_path / 'no_local.pt'), **on_kw).run()
    # with the option off or absent: the same chain, the same metric keys, files and checkpoint keys as without the feature
    runs = {}
    for name, extra in (('off', {'local_similarity': False}), ('absent', {})):
        torch.manual_seed(0)
        runs[name] = make_trainer(tmp_path / name, (N, N, N), **kw, **extra)
        runs[name].run()
    off, absent = runs['off'], runs['absent']
    assert torch.equal(off.v_curr_state, absent.v_curr_state) and torch.equal(off.v_curr_state, a.v_curr_state)
    assert torch.equal(off.displacement_mean, a.displacement_mean) and torch.equal(off.displacement_std, a.displacement_std)
    off_keys = list(off.metrics.result())
    assert off_keys == list(absent.metrics.result()) and not [k for k in off_keys if 'local_similarity' in k]
    assert [k for k in res if 'local_similarity' not in k] == off_keys and sorted(res) == sorted(off_keys + new)
    for t in (off, absent):
        assert t.local_options is None and t._local_similarity is None and t.local_similarity_summary is None
        assert t._local_ranges is None and t.local_lncc_mean is None
    names = lambda tr: sorted(p.name for p in tr.config.save_dirs['samples'].iterdir())
    new_files = ([f'MCMC_lncc_{name}{tail}.nii.gz' for name in ('mean', 'min') for tail in ('', '_masked')] +
                 ['MCMC_lncc_of_mean.nii.gz', 'MCMC_ssim_of_mean.nii.gz'])
    assert names(a) == sorted(names(off) + new_files) and names(off) == names(absent)
    sd_off = torch.load(off.config.save_dirs['checkpoints'] / 'checkpoint_0000006.pt', map_location='cpu', weights_only=True)
    assert set(sd_off) == set(sd)
