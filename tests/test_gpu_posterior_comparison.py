"""Posterior comparison on the device: the known answers and random cases against the numpy restatement, the summary
reduction, non-finite states, determinism, the ABI and Python refusals, and the trainer option end to end (maps against the
recorded displacements of both stages, the VI side against the trainer's own VI displacement std, files, metrics, checkpoint /
resume, and nothing changed when it is off).

Every plane is compared at every finite voxel with the float64 restatement of tests/_posterior_comparison.py evaluated on the
device's own float32 states: shift and log_std_ratio to one float32 ulp, bures (as squares) and jeffreys to the bound forms of
that module with the constants C_B and C_J measured there on the CPU.  The tests print the worst error / tolerance before
they assert.

Measured on one MI355X, worst error / tolerance over all cases: shift 0 ulp, log_std_ratio 0 ulp, bures 0.27, jeffreys 0.21;
the trainer's states against the float64 Welford of the spied records 0.07, the VI diagonal against VI_displacement_std^2 0.08
("Posterior comparison")."""
import copy
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

from ir_sgmcmc_amd import _lib as L
from ir_sgmcmc_amd.diagnostics import COMPARISON_METRICS, DisplacementCovariance, PosteriorComparison, recorded_steps
from ir_sgmcmc_amd.parse_config import ConfigParser
from ir_sgmcmc_amd.posterior_comparison import comparison_summary, posterior_compare
from ir_sgmcmc_amd.trainer import Trainer
from ir_sgmcmc_amd.utils import calc_posterior_comparison
from tests import _posterior_comparison as P
from tests._displacement_covariance import FACTOR, U, covariance_np, matrices

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAINS = {4: 2, 6: 3, 8: 4, 40: 8}  # records of a side -> chains per recorded step


def record_sides(records_a, records_b):
    """both sides through DisplacementCovariance.record, C chains per step -> PosteriorComparison"""
    pc = PosteriorComparison(records_a.shape[2:], DEV)
    for take, rec in ((pc.record_vi, records_a), (pc.record, records_b)):
        Cn = CHAINS[rec.shape[0]]
        t = torch.from_numpy(rec).to(DEV)
        for s in range(rec.shape[0] // Cn):
            take(t[s * Cn:(s + 1) * Cn].contiguous())
    assert (pc.vi.records, pc.mcmc.records, pc.records) == (records_a.shape[0], records_b.shape[0], records_b.shape[0])
    return pc


def states_np(pc):
    return tuple(x.cpu().numpy() for x in (pc.vi.mean, pc.vi.comoment, pc.mcmc.mean, pc.mcmc.comoment))


def planes_np(maps):
    return {k: maps[k].cpu().numpy() for k in P.PLANES}


def check_against_restatement(pc, maps, summary, scale, mask, label='', std_floor=P.STD_FLOOR):
    """planes against the restatement of the device's states; the summary against the restatement of the device's planes"""
    ref = P.compare_np(*states_np(pc)[:2], pc.vi.records, *states_np(pc)[2:], pc.mcmc.records, scale, std_floor)
    planes = planes_np(maps)
    figures = P.check_planes(ref, planes, label)
    want = P.summary_np(planes, ref['tr_a'], ref['tr_b'], ref['floored'], pc.vi.records, pc.mcmc.records, mask)
    P.check_summary(summary, want)
    return ref, planes, figures


def test_known_answers():
    shape = (4, 5, 6)
    ma, Ma, mb, Mb, which = P.known_states(shape)
    dev = lambda x: torch.from_numpy(x).to(DEV)
    *planes, isum, fsum = posterior_compare(dev(ma), dev(Ma), P.KNOWN_N[0], dev(mb), dev(Mb), P.KNOWN_N[1], (1.0, 1.0, 1.0), 1e-3)
    planes = {k: p.cpu().numpy() for k, p in zip(P.PLANES, planes)}
    for k, p in planes.items():
        assert p.dtype == np.float32 and p.shape == shape, k
    P.check_known(planes, None, which)
    same = which == list(P.KNOWN).index('identical')
    assert not planes['shift'][same].any() and not planes['log_std_ratio'][same].any()  # exactly 0
    ref = P.compare_np(ma, Ma, P.KNOWN_N[0], mb, Mb, P.KNOWN_N[1], (1.0, 1.0, 1.0))
    P.check_planes(ref, planes, 'known')
    s = comparison_summary(isum.cpu().tolist(), fsum.cpu().tolist(), *P.KNOWN_N)
    assert (s['voxels'], s['nonfinite_voxels'], s['floored_voxels']) == (120, 0, 30)  # the rank-one case floors four eigenvalues
    assert isum.cpu().tolist()[3] == 30 and s['frac_vi_narrower'] == 0.25              # and is the one with A the narrower
    P.check_summary(s, P.summary_np(planes, ref['tr_a'], ref['tr_b'], ref['floored'], *P.KNOWN_N))
    assert s['shift_max'] == 3.0 and s['w2_max'] == pytest.approx(math.sqrt(13.0), rel=1e-6)  # the rank-one pair: no shift, bures^2 = 13


@pytest.mark.parametrize('with_mask', [False, True])
@pytest.mark.parametrize('recipe', P.RECIPES)
@pytest.mark.parametrize('n_a,n_b', P.RECORDS)
@pytest.mark.parametrize('shape', P.SHAPES)
def test_random_cases_match_the_restatement(shape, n_a, n_b, recipe, with_mask):
    a, b = P.draw_pair(recipe, shape, n_a, n_b)
    pc = record_sides(a, b)
    mask = P.case_mask(shape) if with_mask else None
    maps, summary = pc.finalize(None if mask is None else torch.from_numpy(mask).to(DEV))
    ref, planes, _ = check_against_restatement(pc, maps, summary, P.default_scale(shape), mask, f'{recipe} {shape} {n_a} vs {n_b}')
    assert ref['finite'].all() and summary['nonfinite_voxels'] == 0
    if recipe == 'rank-one':
        assert summary['floored_voxels'] == summary['voxels']
    # the same records against themselves: exactly no shift and no ratio, the other two inside their tolerances of 0
    same = record_sides(a, a)
    maps0, s0 = same.finalize()
    assert not maps0['shift'].any() and not maps0['log_std_ratio'].any()
    check_against_restatement(same, maps0, s0, P.default_scale(shape), None, 'identical')


@pytest.mark.parametrize('recipe', P.RECIPES)
def test_a_scale_of_its_own_a_floor_of_its_own_and_the_functional_form(recipe):
    shape = P.SHAPES[0]
    a, b = P.draw_pair(recipe, shape, *P.RECORDS[0])
    pc = record_sides(a, b)
    maps, summary = pc.finalize(None, P.OWN_SCALE)
    check_against_restatement(pc, maps, summary, P.OWN_SCALE, None, f'{recipe} own scale')
    maps_f, summary_f = pc.finalize(None, P.OWN_SCALE, 0.25)
    check_against_restatement(pc, maps_f, summary_f, P.OWN_SCALE, None, f'{recipe} own floor', std_floor=0.25)
    assert torch.equal(maps_f['shift'], maps['shift']) and torch.equal(maps_f['bures'], maps['bures'])  # neither knows the floor
    mask = torch.from_numpy(P.case_mask(shape)).to(DEV)
    maps2, s2 = calc_posterior_comparison(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), mask, P.OWN_SCALE)
    for k in P.PLANES:
        assert torch.equal(maps2[k].view(torch.int32), maps[k].view(torch.int32)), k
    assert s2['voxels'] == int(mask.sum()) and s2['records_vi'] == a.shape[0] and s2['records_mcmc'] == b.shape[0]


# 263 blocks of partials: threads 0 .. 6 of the second stage fold two blocks each, and V % 256 != 0; 270 400 voxels: more than
# 1024 blocks x 256, so the first stage's grid-stride loop wraps, with a ragged tail.  The smallest shapes on either path.
@pytest.mark.parametrize('shape', [(41, 40, 41), (65, 64, 65)])
def test_summary_reduction_past_one_round_of_either_stage(shape):
    a, b = P.draw_pair('anisotropic', shape, 4, 4)
    pc = record_sides(a, b)
    for mask in (P.case_mask(shape), None):
        maps, summary = pc.finalize(None if mask is None else torch.from_numpy(mask).to(DEV))
        print(summary)
        assert summary['nonfinite_voxels'] == 0 and 0 < summary['frac_vi_narrower'] < 1
        ref = P.compare_np(*states_np(pc)[:2], 4, *states_np(pc)[2:], 4, P.default_scale(shape))
        planes = planes_np(maps)
        P.check_summary(summary, P.summary_np(planes, ref['tr_a'], ref['tr_b'], ref['floored'], 4, 4, mask))


def test_non_finite_states_and_an_empty_mask():
    shape = (4, 5, 6)
    a, b = P.draw_pair('anisotropic', shape, 4, 6)
    pc = record_sides(a, b)
    pc.vi.mean[1, 0, 0, 0] = float('nan')
    pc.mcmc.comoment[4, 1, 2, 3] = float('inf')
    pc.vi.comoment[0, 3, 4, 5] = float('-inf')
    bad = np.zeros(shape, dtype=bool)
    bad[0, 0, 0] = bad[1, 2, 3] = bad[3, 4, 5] = True
    mask = np.ones(shape, dtype=bool)
    mask[3, 4, 5] = False
    maps, s = pc.finalize(torch.from_numpy(mask).to(DEV))
    ref, planes, _ = check_against_restatement(pc, maps, s, P.default_scale(shape), mask, 'non-finite')
    assert np.array_equal(~ref['finite'], bad) and s['voxels'] == 119 and s['nonfinite_voxels'] == 2
    for k in P.PLANES:
        assert np.array_equal(np.isnan(planes[k]), bad), k  # NaN exactly there
    maps0, s0 = pc.finalize(torch.zeros(shape, device=DEV, dtype=torch.bool))
    assert s0['voxels'] == 0 and s0['nonfinite_voxels'] == 0 and s0['floored_voxels'] == 0
    assert all(math.isnan(s0[k]) for k in P.FLOAT_KEYS)
    for k in P.PLANES:
        assert np.array_equal(maps0[k].cpu().numpy(), planes[k], equal_nan=True), k  # the maps do not depend on the mask
    _, s1 = pc.finalize(torch.from_numpy(bad).to(DEV))  # no masked voxel is finite
    assert s1['voxels'] == 3 and s1['nonfinite_voxels'] == 3 and all(math.isnan(s1[k]) for k in P.FLOAT_KEYS)


def test_two_calls_are_bit_identical_and_a_swap_stays_inside_the_tolerance():
    shape = (37, 41, 43)  # more than one block of partials
    a, b = P.draw_pair('anisotropic', shape, 4, 6)
    pc = record_sides(a, b)
    mask = torch.from_numpy(np.random.default_rng(2).random(shape) < 0.3).to(DEV)
    scale = pc.mcmc.default_scale()
    args = (pc.vi.mean, pc.vi.comoment, 4, pc.mcmc.mean, pc.mcmc.comoment, 6, scale, 1e-3, mask)
    r1, r2 = posterior_compare(*args), posterior_compare(*args)
    for u, v in zip(r1, r2):
        assert torch.equal(u.view(torch.uint8), v.view(torch.uint8))
    assert r1[4].dtype == torch.int64 and int(r1[4][0]) == int(mask.sum()) and r1[5].dtype == torch.float64
    assert tuple(r1[4].shape) == (L.IRS_COMPARE_SUMMARY_INTS,) and tuple(r1[5].shape) == (L.IRS_COMPARE_SUMMARY_FLOATS,)
    # B against A.  shift is symmetric and log_std_ratio antisymmetric bit for bit, by construction; bures and jeffreys are formed
    # in B's eigenbasis, so a swap is held to the tolerances, not to the bits
    sw = posterior_compare(pc.mcmc.mean, pc.mcmc.comoment, 6, pc.vi.mean, pc.vi.comoment, 4, scale, 1e-3, mask)
    assert torch.equal(sw[0], r1[0]) and torch.equal(sw[1], -r1[1])
    ref = P.compare_np(*states_np(pc)[:2], 4, *states_np(pc)[2:], 6, scale)
    swapped = {'shift': sw[0].cpu().numpy(), 'log_std_ratio': -sw[1].cpu().numpy(), 'bures': sw[2].cpu().numpy(),
               'jeffreys': sw[3].cpu().numpy()}
    P.check_planes(ref, swapped, 'swapped')
    assert int(sw[4][3]) + int(r1[4][3]) == int(r1[4][0])  # no ratio is exactly 0 here: narrower on one side or the other


def test_abi_and_python_refusals():
    lib = L.load()
    D, H, W = 4, 5, 6
    a, b = P.draw_pair('anisotropic', (D, H, W), 4, 6)
    pc = record_sides(a, b)
    ma, Ma, mb, Mb = pc.vi.mean, pc.vi.comoment, pc.mcmc.mean, pc.mcmc.comoment
    SENTINEL = -7.0
    planes = [torch.full((D, H, W), SENTINEL, device=DEV) for _ in range(4)]
    isum = torch.full((L.IRS_COMPARE_SUMMARY_INTS,), -7, device=DEV, dtype=torch.int64)
    fsum = torch.full((L.IRS_COMPARE_SUMMARY_FLOATS,), SENTINEL, device=DEV, dtype=torch.float64)
    ws = torch.empty(L.IRS_COMPARE_WS_BYTES, device=DEV, dtype=torch.uint8)
    q = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    st = L.stream_ptr()
    good = (C.c_float * 3)(1.0, 1.0, 1.0)

    def call(ma_=ma, Ma_=Ma, n_a=4, mb_=mb, Mb_=Mb, n_b=6, D_=D, H_=H, W_=W, scale=good, floor=1e-3, p0=planes[0], p1=planes[1],
             p2=planes[2], p3=planes[3], isum_=isum, fsum_=fsum, ws_=ws, ws_bytes=L.IRS_COMPARE_WS_BYTES):
        return lib.irs_posterior_compare(q(ma_), q(Ma_), n_a, q(mb_), q(Mb_), n_b, D_, H_, W_, scale, floor, None, q(p0), q(p1), q(p2),
                                         q(p3), q(isum_), q(fsum_), q(ws_), ws_bytes, st)

    bad_scales = [(C.c_float * 3)(*s) for s in ((0.0, 1, 1), (1, -2.0, 1), (1, 1, float('nan')), (float('inf'), 1, 1))]
    for kw in (dict(ma_=None), dict(Ma_=None), dict(mb_=None), dict(Mb_=None), dict(scale=None), dict(p0=None), dict(p1=None),
               dict(p2=None), dict(p3=None), dict(isum_=None), dict(fsum_=None), dict(ws_=None), dict(D_=1), dict(H_=1), dict(W_=0),
               dict(n_a=1), dict(n_b=1), dict(n_a=0), dict(n_b=-3), dict(floor=0.0), dict(floor=-1e-3), dict(floor=float('nan')),
               dict(floor=float('inf')), dict(ws_bytes=L.IRS_COMPARE_WS_BYTES - 1), dict(ws_bytes=0),
               *(dict(scale=s) for s in bad_scales)):
        with pytest.raises(L.IrsError):
            L.check(call(**kw))
    torch.cuda.synchronize()
    for p in planes:  # a refused call has written nothing
        assert bool((p == SENTINEL).all())
    assert bool((isum == -7).all()) and bool((fsum == SENTINEL).all())
    L.check(call())
    torch.cuda.synchronize()
    assert isum.cpu().tolist()[:2] == [D * H * W, 0] and not any(bool((p == SENTINEL).any()) for p in planes)
    # the Python surface checks dtypes, shapes, devices and numbers before it calls
    sc = (1.0, 1.0, 1.0)
    f = posterior_compare
    for bad in (lambda: f(ma.double(), Ma, 4, mb, Mb, 6, sc), lambda: f(ma, Ma, 4, mb, Mb.double(), 6, sc),
                lambda: f(ma.cpu(), Ma.cpu(), 4, mb.cpu(), Mb.cpu(), 6, sc), lambda: f(ma, Ma, 4, mb.cpu(), Mb, 6, sc),
                lambda: f(ma[0], Ma[0], 4, mb[0], Mb[0], 6, sc), lambda: f(ma, Ma[:5], 4, mb, Mb, 6, sc),
                lambda: f(ma, Ma, 4, mb[..., :5], Mb[..., :5], 6, sc), lambda: f(ma, Ma, 4, mb[:2], Mb, 6, sc),
                lambda: f(ma, Ma, 1, mb, Mb, 6, sc), lambda: f(ma, Ma, 4, mb, Mb, 1, sc), lambda: f(ma, Ma, 4.5, mb, Mb, 6, sc),
                lambda: f(ma, Ma, 4, mb, Mb, 6, (1.0, 1.0)), lambda: f(ma, Ma, 4, mb, Mb, 6, (1.0, 0.0, 1.0)),
                lambda: f(ma, Ma, 4, mb, Mb, 6, sc, 0.0), lambda: f(ma, Ma, 4, mb, Mb, 6, sc, float('nan')),
                lambda: f(ma, Ma, 4, mb, Mb, 6, sc, '1e-3'),
                lambda: f(ma, Ma, 4, mb, Mb, 6, sc, mask=torch.ones(D, H, W + 1, device=DEV, dtype=torch.bool)),
                lambda: f(ma, Ma, 4, mb, Mb, 6, sc, mask=torch.ones(D, H, W, device=DEV))):
        with pytest.raises(L.IrsError):
            bad()
    one = PosteriorComparison((D, H, W), DEV)
    one.record_vi(torch.from_numpy(a[:1]).to(DEV))
    one.record(torch.from_numpy(b).to(DEV)[:3].contiguous())
    with pytest.raises(RuntimeError, match='1 records on the VI side'):
        one.finalize()
    with pytest.raises(ValueError, match='different grids'):
        calc_posterior_comparison(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)[..., :5].contiguous())


# ---------------------------------------------------------------- the trainer option
def make_trainer(tmp_path, dims, **trainer_over):
    cfg = json.load(open(os.path.join(ROOT, 'configs', 'synthetic_gmm_lognormal.json')))
    cfg['trainer']['save_dir'] = str(tmp_path)
    cfg['data_loader']['args']['dims'] = list(dims)
    cfg['trainer'].update(trainer_over)
    config = ConfigParser.from_dict(copy.deepcopy(cfg), timestamp='t')
    dl = config.init_data_loader()
    losses = config.init_losses()
    tm, rm = config.init_transformation_and_registration_modules()
    return Trainer(config, dl, losses, tm, rm, config.init_metrics(), device=DEV)


RUN = dict(VI=True, no_iters_VI=2, no_samples_VI_test=4, log_period_VI=1, no_chains=2, no_iters_burn_in=2, no_samples_MCMC=8)
NEW_FILES = [f'MCMC_vs_VI_{name}{tail}.nii.gz' for name in P.PLANES for tail in ('', '_masked')]


def check_state(dc, records, scale):
    """a side's float32 state against the float64 one of the spied records: |S32 - S|_F <= E (tests/_displacement_covariance.py)"""
    ref = covariance_np(records, scale=scale)
    dS = matrices(dc.comoment.cpu().numpy(), records.shape[0], scale) - ref['S']
    err = np.sqrt((dS ** 2).sum(axis=(-1, -2)))
    print({'state |S32 - S|_F': (float(err.max()), float((err / np.maximum(ref['E'], 1e-300)).max()))})
    assert (err <= ref['E']).all()
    assert np.abs(dc.mean.cpu().numpy() - ref['mean']).max() <= 17 * U * np.abs(records).max()
    return ref


def test_trainer_maps_match_the_recorded_displacements(tmp_path, monkeypatch):
    from ir_sgmcmc_amd.utils.imageio import read_nifti
    N = 16
    kept = {'vi': [], 'mcmc': []}
    record_vi, record = PosteriorComparison.record_vi, PosteriorComparison.record

    def spy_vi(self, displacement):
        kept['vi'].append(displacement.clone())
        return record_vi(self, displacement)

    def spy(self, displacement):
        kept['mcmc'].append(displacement.clone())
        return record(self, displacement)

    monkeypatch.setattr(PosteriorComparison, 'record_vi', spy_vi)
    monkeypatch.setattr(PosteriorComparison, 'record', spy)
    kw = dict(RUN, log_period_MCMC=2, checkpoint_period=6)
    torch.manual_seed(0)
    t = make_trainer(tmp_path / 'on', (N, N, N), posterior_comparison={'period': 2}, **kw)
    t.run()
    pc = t._posterior_comparison
    assert len(kept['vi']) == 4 and len(kept['mcmc']) == len(recorded_steps(2, 8, 2)) == 4
    assert (pc.vi.records, pc.mcmc.records) == (4, 8)
    rec_vi, rec_mcmc = (torch.cat(kept[k]).cpu().numpy() for k in ('vi', 'mcmc'))  # in order; chains in order within a step
    assert rec_vi.shape == (4, 3, N, N, N) and rec_mcmc.shape == (8, 3, N, N, N)
    batch = next(iter(t.data_loader))
    mask = batch[1].get('mask', batch[0]['mask']).reshape(N, N, N).numpy() != 0
    scale = P.default_scale((N, N, N))
    # the states are those of the spied records, and the maps those of the states
    ref_vi = check_state(pc.vi, rec_vi, scale)
    check_state(pc.mcmc, rec_mcmc, scale)
    maps = {k: getattr(t, f'comparison_{k}') for k in P.PLANES}
    _, planes, _ = check_against_restatement(pc, maps, t.comparison_summary, scale, mask, 'trainer')
    s = t.comparison_summary
    assert (s['records_vi'], s['records_mcmc'], s['voxels'], s['nonfinite_voxels']) == (4, 8, int(mask.sum()), 0)
    # the VI side's diagonal against the trainer's own VI displacement std: the covariance test's bound (twice FACTOR dM_aa
    # for two evaluations of the same records, 4 u for the division and the square root)
    var = pc.vi.covariance()[:3].cpu().numpy().astype(np.float64)
    var_t = t.VI_displacement_std.cpu().numpy().astype(np.float64) ** 2
    tol = 2 * FACTOR * ref_vi['dM'][:3] / 3 + 4 * U * var_t
    err = np.abs(var - var_t)
    print({'VI variance against Trainer.VI_displacement_std^2': (float(err.max()), float((err / tol).max()))})
    assert (err <= tol).all()
    # files
    folder = t.config.save_dirs['samples']
    for name in P.PLANES:
        plain, _ = read_nifti(str(folder / f'MCMC_vs_VI_{name}.nii.gz'))
        assert np.array_equal(plain, planes[name])
        masked, _ = read_nifti(str(folder / f'MCMC_vs_VI_{name}_masked.nii.gz'))
        assert np.array_equal(masked[mask], planes[name][mask]) and not masked[~mask].any()
    # metrics
    res = t.metrics.result()
    for k in COMPARISON_METRICS:
        got, want = res[f'MCMC/vs_VI/{k}'], s[k]
        assert (math.isnan(got) and math.isnan(want)) or got == want
    # the same run with the option off: bit-identical chains and moments of both stages, and no comparison anything
    monkeypatch.setattr(PosteriorComparison, 'record_vi', record_vi)
    monkeypatch.setattr(PosteriorComparison, 'record', record)
    torch.manual_seed(0)
    off = make_trainer(tmp_path / 'off', (N, N, N), **kw)
    off.run()
    for name in ('v_curr_state', 'displacement_mean', 'displacement_std', 'VI_displacement_mean', 'VI_displacement_std'):
        assert torch.equal(getattr(off, name), getattr(t, name)), name
    assert off._posterior_comparison is None and off.comparison_summary is None and off.comparison_shift is None
    assert off.comparison_log_std_ratio is None and off.comparison_bures is None and off.comparison_jeffreys is None
    on_keys, off_keys = list(res), list(off.metrics.result())
    assert not [k for k in off_keys if k.startswith('MCMC/vs_VI/')]
    assert [k for k in on_keys if not k.startswith('MCMC/vs_VI/')] == off_keys
    assert [k for k in on_keys if k.startswith('MCMC/vs_VI/')] == [f'MCMC/vs_VI/{k}' for k in COMPARISON_METRICS]
    names = lambda tr: sorted(p.name for p in tr.config.save_dirs['samples'].iterdir())
    assert names(t) == sorted(names(off) + NEW_FILES)
    load = lambda tr: torch.load(tr.config.save_dirs['checkpoints'] / 'checkpoint_0000006.pt', map_location='cpu', weights_only=True)
    sd_on, sd_off = load(t), load(off)
    assert set(sd_on) == set(sd_off) | {'posterior_comparison'}
    assert torch.equal(sd_on['v_curr_state'], sd_off['v_curr_state'])


def test_trainer_posterior_comparison_survives_checkpoint_resume_bit_for_bit(tmp_path):
    kw = dict(RUN, log_period_MCMC=4, checkpoint_period=6, posterior_comparison={'period': 2}, save_outputs=False)
    torch.manual_seed(0)
    a = make_trainer(tmp_path / 'a', (16, 16, 16), **kw)
    a.run()
    ck = a.config.save_dirs['checkpoints'] / 'checkpoint_0000006.pt'
    sd = torch.load(ck, map_location='cpu', weights_only=True)
    assert sd['posterior_comparison']['vi']['records'] == 4 and sd['posterior_comparison']['mcmc']['records'] == 2 * a.no_chains
    assert tuple(sd['posterior_comparison']['vi']['comoment'].shape) == (6, 16, 16, 16)

    def same_as_a(other):
        for name in P.PLANES:
            x, y = getattr(a, f'comparison_{name}'), getattr(other, f'comparison_{name}')
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), name
        for side in ('vi', 'mcmc'):
            for name in ('mean', 'comoment'):
                assert torch.equal(getattr(getattr(a._posterior_comparison, side), name),
                                   getattr(getattr(other._posterior_comparison, side), name)), (side, name)
        assert json.dumps(a.comparison_summary, sort_keys=True) == json.dumps(other.comparison_summary, sort_keys=True)

    # the VI stage runs again, under another seed: its records are replaced by the checkpoint's
    torch.manual_seed(1)
    b = make_trainer(tmp_path / 'b', (16, 16, 16), resume=str(ck), **kw)
    b.run()
    same_as_a(b)
    # no VI stage at all: the VI side is the checkpoint's
    c = make_trainer(tmp_path / 'c', (16, 16, 16), resume=str(ck), **dict(kw, VI=False))
    c.run()
    assert c._posterior_comparison.vi.records == 4
    same_as_a(c)
    # states of other dims are refused; a checkpoint without the key, once a recorded step has passed, too
    with pytest.raises(ValueError, match='shape'):
        PosteriorComparison((16, 16, 17), DEV).load_state_dict(sd['posterior_comparison'])
    del sd['posterior_comparison']
    ck2 = tmp_path / 'no_comparison.pt'
    torch.save(sd, ck2)
    d = make_trainer(tmp_path / 'd', (16, 16, 16), resume=str(ck2), **dict(kw, VI=False))
    with pytest.raises(ValueError, match='posterior_comparison'):
        d.run()
    assert isinstance(a._posterior_comparison.mcmc, DisplacementCovariance)
