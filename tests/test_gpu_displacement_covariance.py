"""Displacement covariance posterior on the device: the known answers and random cases against the numpy restatement, the
summary reduction, determinism, one launch of C chains against C launches of one, the ABI and Python refusals, and the trainer
option end to end (maps against the recorded displacements, the diagonal against the trainer's own displacement std, files,
metrics, checkpoint / resume, and nothing changed when it is off).

Every map is compared at every finite voxel against the tolerances of tests/_displacement_covariance.py: a forward bound E on
the float32 state, carried through Weyl, the residual identity, Davis-Kahan and the anisotropy's Lipschitz constant.  Only the
comparison with the reference eigenvector leaves voxels out (relative gap below 0.05, at most 0.5 % of them, asserted);
test_displacement_covariance_host.py checks on the CPU that a float32 evaluation of the same inputs stays inside them.

Measured on one MI355X, worst error / tolerance over all cases: state 0.13, eigenvalues 0.11, direction norm 0.21, direction
residual 0.06, eigenvector sine 0.03, anisotropy 0.012."""
import copy
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

from ir_sgmcmc_amd import _lib as L
from ir_sgmcmc_amd import ops
from ir_sgmcmc_amd.diagnostics import COVARIANCE_METRICS, DisplacementCovariance, recorded_steps
from ir_sgmcmc_amd.parse_config import ConfigParser
from ir_sgmcmc_amd.trainer import Trainer
from ir_sgmcmc_amd.utils import calc_displacement_covariance
from tests._displacement_covariance import (CASES, FACTOR, HAND_FA, HAND_STD, RECIPES, U, case_mask, case_seed, check_maps,
                                            covariance_np, draw_records, hand_checked_records, summary_np)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_KEYS = ('records', 'voxels', 'nonfinite_voxels')
FLOAT_KEYS = ('std_major_mean', 'std_major_max', 'std_total_mean', 'anisotropy_mean', 'anisotropy_max', 'dir_x', 'dir_y', 'dir_z')


def run_device(records, C, mask=None, scale=None):
    """records (n,3,D,H,W) float32 in record order, C chains per step -> (DisplacementCovariance, std, direction, anisotropy
    as numpy, summary)"""
    n = records.shape[0]
    assert n % C == 0
    dc = DisplacementCovariance(records.shape[2:], DEV)
    rec = torch.from_numpy(records).to(DEV)
    for s in range(n // C):
        dc.record(rec[s * C:(s + 1) * C].contiguous())
    m = None if mask is None else torch.from_numpy(mask).to(DEV)
    std, d, fa, summary = dc.finalize(m, scale)
    return dc, std.cpu().numpy(), d.cpu().numpy(), fa.cpu().numpy(), summary


def check_state(dc, ref):
    """the float32 state against the float64 one: |S32 - S|_F <= E at every finite voxel (E is what everything else rests on)"""
    n, scale, fin = ref['n'], ref['scale'], ref['finite']
    from tests._displacement_covariance import matrices
    M = dc.comoment.cpu().numpy()
    assert np.array_equal(np.isfinite(M).all(axis=0) & np.isfinite(dc.mean.cpu().numpy()).all(axis=0), fin)
    dS = (matrices(np.where(fin, M, 0.0), n, scale) - ref['S'])[fin]
    err = np.sqrt((dS ** 2).sum(axis=(-1, -2)))
    E = ref['E'][fin]
    print({'state |S32 - S|_F': (float(err.max()) if err.size else 0.0, float((err / np.maximum(E, 1e-300)).max()) if err.size else 0.0)})
    assert (err <= E).all()


def check_summary(summary, n, std, d, fa, mask):
    """integers exactly, floats against the restatement of the DEVICE's stored maps (this pins the reduction)"""
    want = summary_np(n, std, d, fa, mask)
    for key in INT_KEYS:
        assert summary[key] == want[key], (key, summary[key], want[key])
    for key in FLOAT_KEYS:
        g, w = summary[key], want[key]
        assert (math.isnan(g) and math.isnan(w)) or abs(g - w) <= 1e-6 * abs(w), (key, g, w)


@pytest.mark.parametrize('rotate', [False, True])
def test_known_answers(rotate):
    records = hand_checked_records(rotate=rotate)
    dc, std, d, fa, s = run_device(records, 2, scale=(1, 1, 1))
    assert dc.records == 4 and np.abs(dc.mean.cpu().numpy()).max() <= 1e-7
    for i in range(3):
        assert np.abs(std[i] - HAND_STD[i]).max() <= 1e-6
    want = (math.sqrt(0.5), math.sqrt(0.5), 0.0) if rotate else (1.0, 0.0, 0.0)
    for i in range(3):
        assert np.abs(d[i] - want[i]).max() <= 1e-6
    assert np.abs(fa - HAND_FA).max() <= 1e-6
    assert (s['records'], s['voxels'], s['nonfinite_voxels']) == (4, 60, 0)
    assert s['std_major_max'] == pytest.approx(HAND_STD[0], abs=1e-6) and s['anisotropy_mean'] == pytest.approx(HAND_FA, abs=1e-6)
    assert s['dir_x'] == pytest.approx(want[0], abs=1e-6) and s['dir_y'] == pytest.approx(want[1], abs=1e-6) and s['dir_z'] == 0.0
    ref = covariance_np(records, scale=(1, 1, 1))
    check_state(dc, ref)
    check_maps(ref, std, d, fa)
    check_summary(s, 4, std, d, fa, None)


def test_one_record_gives_zero_everywhere():
    records = draw_records('anisotropic', 1, (4, 5, 6), 9)
    dc, std, d, fa, s = run_device(records, 1)
    assert torch.equal(dc.mean.cpu(), torch.from_numpy(records[0])) and not dc.comoment.any()
    assert not std.any() and not d.any() and not fa.any()
    assert not np.signbit(d).any()  # the zero vector, not its negative
    assert s['records'] == 1 and s['voxels'] == 120 and s['std_major_max'] == 0.0 and s['anisotropy_max'] == 0.0 and s['dir_x'] == 0.0


@pytest.mark.parametrize('with_mask', [False, True])
@pytest.mark.parametrize('recipe', RECIPES)
@pytest.mark.parametrize('C,steps,shape', CASES)
def test_random_cases_match_the_restatement(C, steps, shape, recipe, with_mask):
    n = C * steps
    records = draw_records(recipe, n, shape, case_seed(C, steps, shape, recipe))
    mask = case_mask(shape) if with_mask else None
    dc, std, d, fa, s = run_device(records, C, mask)
    assert dc.records == n
    ref = covariance_np(records, mask=mask)
    check_state(dc, ref)
    check_maps(ref, std, d, fa, compare_eigenvector=recipe == 'anisotropic', all_fa=n >= 2)
    check_summary(s, n, std, d, fa, mask)


# 263 blocks of partials: threads 0 .. 6 of the second stage fold two blocks each, and V % 256 != 0; 270 400 voxels: more than
# 1024 blocks x 256, so the first stage's grid-stride loop wraps, with a ragged tail.  The smallest shapes on either path.
@pytest.mark.parametrize('shape', [(41, 40, 41), (65, 64, 65)])
def test_summary_reduction_past_one_round_of_either_stage(shape):
    records = draw_records('anisotropic', 3, shape, case_seed(3, 1, shape, 'anisotropic'))
    dc = DisplacementCovariance(shape, DEV)
    dc.record(torch.from_numpy(records).to(DEV).contiguous())
    for mask in (case_mask(shape), None):
        std, d, fa, summary = dc.finalize(None if mask is None else torch.from_numpy(mask).to(DEV))
        print(summary)
        assert summary['nonfinite_voxels'] == 0  # every masked voxel enters the float columns
        check_summary(summary, 3, std.cpu().numpy(), d.cpu().numpy(), fa.cpu().numpy(), mask)


def test_a_scale_of_its_own_and_the_covariance_tensor():
    shape = (9, 6, 70)
    records = draw_records('anisotropic', 6, shape, 31)
    scale = (1.5, 0.25, 40.0)
    dc, std, d, fa, s = run_device(records, 3, scale=scale)
    ref = covariance_np(records, scale=scale)
    check_state(dc, ref)
    check_maps(ref, std, d, fa, max_gap_share=1.0)
    # covariance(): M / max(n - 1, 1) in normalised units; its diagonal against an independent float64 variance
    cov = dc.covariance()
    assert tuple(cov.shape) == (6,) + shape and cov.dtype == torch.float32
    var = records.astype(np.float64).var(axis=0, ddof=1)
    tol = FACTOR * ref['dM'][:3] / 5 + 2 * U * var  # the bound on the state, and the division
    err = np.abs(cov[:3].cpu().numpy().astype(np.float64) - var)
    print({'variance': (float(err.max()), float((err / tol).max()))})
    assert (err <= tol).all()
    x = records.astype(np.float64) - records.astype(np.float64).mean(axis=0)
    xy = (x[:, 0] * x[:, 1]).sum(axis=0) / 5
    assert (np.abs(cov[3].cpu().numpy() - xy) <= FACTOR * ref['dM'][3] / 5 + 2 * U * np.abs(xy)).all()


def test_nan_inputs_and_an_empty_mask():
    shape = (4, 5, 6)
    records = draw_records('anisotropic', 4, shape, 4)
    records[1, 2, 1, 2, 3] = np.nan
    records[2, 0, 3, 4, 5] = np.inf
    records[0, 1, 0, 0, 0] = -np.inf  # in the record that overwrites
    mask = np.ones(shape, dtype=bool)
    mask[3, 4, 5] = False
    dc, std, d, fa, s = run_device(records, 2, mask)
    ref = covariance_np(records, mask=mask)
    assert (~ref['finite']).sum() == 3 and s['nonfinite_voxels'] == 2 and s['voxels'] == 119
    for plane in (*std, *d, fa):
        assert np.isnan(plane[~ref['finite']]).all()
    check_state(dc, ref)
    check_maps(ref, std, d, fa, max_gap_share=1.0)
    check_summary(s, 4, std, d, fa, mask)
    _, std0, d0, fa0, s0 = run_device(records, 2, np.zeros(shape, dtype=bool))
    assert s0['voxels'] == 0 and s0['nonfinite_voxels'] == 0 and all(math.isnan(s0[k]) for k in FLOAT_KEYS)
    assert np.array_equal(std0, std, equal_nan=True)  # the maps do not depend on the mask
    only_bad = ~ref['finite']
    _, _, _, _, s1 = run_device(records, 2, only_bad)  # no masked voxel is finite
    assert s1['voxels'] == 3 and s1['nonfinite_voxels'] == 3 and all(math.isnan(s1[k]) for k in FLOAT_KEYS)


@pytest.mark.parametrize('shape', [(5, 7, 9), (8, 6, 10)])  # V % 4 != 0 and == 0
def test_one_launch_of_c_chains_equals_c_launches_and_a_restart_overwrites(shape):
    records = draw_records('anisotropic', 11, shape, 5)  # more records than one launch folds
    t = torch.from_numpy(records).to(DEV)
    std, d, fa, s = calc_displacement_covariance(t)
    assert s['records'] == 11
    one = DisplacementCovariance(shape, DEV)
    one.mean.fill_(3.0)  # records_before = 0 overwrites whatever the state held
    one.comoment.fill_(float('nan'))
    for r in range(11):
        one.record(t[r:r + 1].contiguous())
    odd = DisplacementCovariance(shape, DEV)
    for lo, hi in ((0, 3), (3, 4), (4, 11)):
        odd.record(t[lo:hi].contiguous())
    for other in (one, odd):
        out = other.finalize()
        for got, want in zip(out[:3], (std, d, fa)):
            assert torch.equal(got.view(torch.int32), want.view(torch.int32))
        assert json.dumps(out[3], sort_keys=True) == json.dumps(s, sort_keys=True)
    assert torch.equal(one.mean, odd.mean) and torch.equal(one.comoment, odd.comoment)
    # the functional form takes a mask and a scale
    mask = torch.from_numpy(case_mask(shape)).to(DEV)
    std2, _, _, s2 = calc_displacement_covariance(t, mask, (2.0, 2.0, 2.0))
    unit = calc_displacement_covariance(t, mask, (1.0, 1.0, 1.0))
    assert s2['voxels'] == int(mask.sum()) and torch.allclose(std2, 2 * unit[0], rtol=1e-6, atol=0)


def test_the_update_does_not_depend_on_the_shape_of_the_volume():
    """the same records as a volume of their own (V % 4 == 0) and as the leading part of a wider, odd one"""
    shape, wide = (6, 5, 8), (6, 5, 9)
    records = draw_records('anisotropic', 6, wide, 17)
    part = np.ascontiguousarray(records[..., :8])
    a = run_device(part, 3, scale=(1, 1, 1))
    b = run_device(records, 3, scale=(1, 1, 1))
    assert torch.equal(a[0].mean, b[0].mean[..., :8]) and torch.equal(a[0].comoment, b[0].comoment[..., :8])
    for x, y in zip(a[1:4], b[1:4]):
        assert np.array_equal(x, y[..., :8])
    assert shape == part.shape[2:]


def test_two_update_sequences_and_two_finalize_calls_are_bit_identical():
    shape = (37, 41, 43)  # more than one block of partials
    records = draw_records('anisotropic', 6, shape, 11)
    mask = np.random.default_rng(2).random(shape) < 0.3
    a = run_device(records, 3, mask)
    b = run_device(records, 3, mask)
    assert torch.equal(a[0].mean, b[0].mean) and torch.equal(a[0].comoment, b[0].comoment)
    for x, y in zip(a[1:4], b[1:4]):
        assert np.array_equal(x, y, equal_nan=True)
    assert json.dumps(a[4], sort_keys=True) == json.dumps(b[4], sort_keys=True)
    m = torch.from_numpy(mask).to(DEV)
    scale = a[0].default_scale()
    r1 = ops.displacement_covariance_finalize(a[0].mean, a[0].comoment, 6, scale, m)
    r2 = ops.displacement_covariance_finalize(a[0].mean, a[0].comoment, 6, scale, m)
    for u, v in zip(r1, r2):
        assert torch.equal(u.view(torch.uint8), v.view(torch.uint8))
    assert r1[3].dtype == torch.int64 and int(r1[3][0]) == int(mask.sum()) and r1[4].dtype == torch.float64
    assert tuple(r1[3].shape) == (L.IRS_COVARIANCE_SUMMARY_INTS,) and tuple(r1[4].shape) == (L.IRS_COVARIANCE_SUMMARY_FLOATS,)


def test_abi_and_python_refusals():
    lib = L.load()
    Cn, D, H, W = 2, 4, 5, 6
    x = torch.from_numpy(draw_records('anisotropic', Cn, (D, H, W), 1)).to(DEV)
    mean = torch.zeros(3, D, H, W, device=DEV)
    com = torch.zeros(6, D, H, W, device=DEV)
    std, d = torch.empty(3, D, H, W, device=DEV), torch.empty(3, D, H, W, device=DEV)
    fa = torch.empty(D, H, W, device=DEV)
    isum = torch.empty(2, device=DEV, dtype=torch.int64)
    fsum = torch.empty(8, device=DEV, dtype=torch.float64)
    ws = torch.empty(L.IRS_COVARIANCE_WS_BYTES, device=DEV, dtype=torch.uint8)
    q = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    st = L.stream_ptr()
    good = (C.c_float * 3)(1.0, 1.0, 1.0)

    def upd(x_=x, C_=Cn, D_=D, mean_=mean, com_=com, before=0):
        return lib.irs_displacement_covariance_update(q(x_), C_, D_, H, W, q(mean_), q(com_), before, st)

    def fin(mean_=mean, com_=com, D_=D, n=2, scale=good, std_=std, d_=d, fa_=fa, isum_=isum, fsum_=fsum, ws_=ws,
            ws_bytes=L.IRS_COVARIANCE_WS_BYTES):
        return lib.irs_displacement_covariance_finalize(q(mean_), q(com_), D_, H, W, n, scale, None, q(std_), q(d_), q(fa_),
                                                        q(isum_), q(fsum_), q(ws_), ws_bytes, st)

    for kw in (dict(x_=None), dict(mean_=None), dict(com_=None), dict(C_=0), dict(C_=9), dict(D_=1), dict(D_=0), dict(before=-1),
               dict(before=2 ** 31 - 2)):
        with pytest.raises(L.IrsError):
            L.check(upd(**kw))
    bad_scales = [(C.c_float * 3)(*s) for s in ((0.0, 1, 1), (1, -2.0, 1), (1, 1, float('nan')), (float('inf'), 1, 1))]
    for kw in (dict(mean_=None), dict(com_=None), dict(scale=None), dict(std_=None), dict(d_=None), dict(fa_=None), dict(isum_=None),
               dict(fsum_=None), dict(ws_=None), dict(D_=1), dict(n=0), dict(n=-1), dict(ws_bytes=8),
               *(dict(scale=s) for s in bad_scales)):
        with pytest.raises(L.IrsError):
            L.check(fin(**kw))
    torch.cuda.synchronize()
    assert float(mean.abs().sum()) == 0.0 and float(com.abs().sum()) == 0.0  # nothing was folded in by a refused call
    L.check(upd())
    L.check(fin())
    torch.cuda.synchronize()
    assert isum.cpu().tolist() == [D * H * W, 0]
    # the Python surface checks dtypes, shapes and devices before it calls
    sc = (1.0, 1.0, 1.0)
    for bad in (lambda: ops.displacement_covariance_update(x.double(), mean, com, 0),
                lambda: ops.displacement_covariance_update(x.cpu(), mean, com, 0),
                lambda: ops.displacement_covariance_update(x[:, :2].contiguous(), mean, com, 0),
                lambda: ops.displacement_covariance_update(x[:, :, :2].contiguous(), mean, com, 0),
                lambda: ops.displacement_covariance_update(x, mean.double(), com, 0),
                lambda: ops.displacement_covariance_update(x, mean, com[:3], 0),
                lambda: ops.displacement_covariance_update(x, mean, com[..., :3], 0),
                lambda: ops.displacement_covariance_update(x, mean.cpu(), com.cpu(), 0),
                lambda: ops.displacement_covariance_finalize(mean, com, 0, sc),
                lambda: ops.displacement_covariance_finalize(mean.cpu(), com.cpu(), 2, sc),
                lambda: ops.displacement_covariance_finalize(mean.double(), com, 2, sc),
                lambda: ops.displacement_covariance_finalize(mean, com[:5], 2, sc),
                lambda: ops.displacement_covariance_finalize(mean[0], com[0], 2, sc),
                lambda: ops.displacement_covariance_finalize(mean, com, 2, (1.0, 1.0)),
                lambda: ops.displacement_covariance_finalize(mean, com, 2, (1.0, 0.0, 1.0)),
                lambda: ops.displacement_covariance_finalize(mean, com, 2, sc, mask=torch.ones(D, H, W + 1, device=DEV, dtype=torch.bool)),
                lambda: ops.displacement_covariance_finalize(mean, com, 2, sc, mask=torch.ones(D, H, W, device=DEV))):
        with pytest.raises(L.IrsError):
            bad()


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


NEW_FILES = ['MCMC_disp_anisotropy.nii.gz', 'MCMC_disp_anisotropy_masked.nii.gz', 'MCMC_disp_direction.vtk',
             'MCMC_disp_std_major.nii.gz', 'MCMC_disp_std_major_masked.nii.gz', 'MCMC_disp_std_minor.nii.gz',
             'MCMC_disp_std_minor_masked.nii.gz']


def test_trainer_maps_match_the_recorded_displacements(tmp_path, monkeypatch):
    from ir_sgmcmc_amd.utils.imageio import read_nifti
    N = 24
    kept = []
    record = DisplacementCovariance.record

    def spy(self, displacement):
        kept.append(displacement.clone())
        return record(self, displacement)

    monkeypatch.setattr(DisplacementCovariance, 'record', spy)
    # burn-in a multiple of the log period: the option's steps are then the steps of the displacement mean / std
    kw = dict(no_chains=2, no_iters_burn_in=4, no_samples_MCMC=8, log_period_MCMC=2)
    torch.manual_seed(0)
    t = make_trainer(tmp_path / 'on', (N, N, N), displacement_covariance=True, **kw)
    t.run()
    C_ = t.no_chains
    n = C_ * 4
    assert C_ == 2 and len(kept) == len(recorded_steps(4, 8, 2)) == 4 and t._displacement_covariance.records == n
    records = torch.cat(kept).cpu().numpy()  # steps in order, chains in order within a step
    batch = next(iter(t.data_loader))
    mask = batch[1].get('mask', batch[0]['mask']).reshape(N, N, N).numpy() != 0
    ref = covariance_np(records, mask=mask)
    std, d, fa = (x.cpu().numpy() for x in (t.displacement_cov_std, t.displacement_cov_direction, t.displacement_cov_anisotropy))
    check_state(t._displacement_covariance, ref)
    # the chains move little in eight transitions: the inputs are what they are, so neither share is asserted here
    check_maps(ref, std, d, fa, max_gap_share=1.0, all_fa=False)
    check_summary(t.displacement_cov_summary, n, std, d, fa, mask)
    # the diagonal of covariance() against the trainer's own displacement std: both are float32 Welford evaluations of the same
    # records in the same order, each within FACTOR dM_aa of the float64 co-moment; the division and the square root add 4 u
    var = t._displacement_covariance.covariance()[:3].cpu().numpy().astype(np.float64)
    var_t = t.displacement_std.cpu().numpy().astype(np.float64) ** 2
    tol = 2 * FACTOR * ref['dM'][:3] / (n - 1) + 4 * U * var_t
    err = np.abs(var - var_t)
    print({'variance against Trainer.displacement_std^2': (float(err.max()), float((err / tol).max()))})
    assert (err <= tol).all()
    # the means: twice Em = u (2 R + X (n + 1) / 2) with R <= 2 X
    assert torch.allclose(t._displacement_covariance.mean, t.displacement_mean, rtol=0, atol=float(17 * U * np.abs(records).max()))
    # files
    folder = t.config.save_dirs['samples']
    for name, im in (('disp_std_major', std[0]), ('disp_std_minor', std[2]), ('disp_anisotropy', fa)):
        plain, _ = read_nifti(str(folder / f'MCMC_{name}.nii.gz'))
        assert np.array_equal(plain, im)
        masked, _ = read_nifti(str(folder / f'MCMC_{name}_masked.nii.gz'))
        assert np.array_equal(masked[mask], im[mask]) and not masked[~mask].any()
    assert (folder / 'MCMC_disp_direction.vtk').stat().st_size > 3 * N ** 3
    # metrics
    res = t.metrics.result()
    for k in COVARIANCE_METRICS:
        got, want = res[f'MCMC/covariance/{k}'], t.displacement_cov_summary[k]
        assert (math.isnan(got) and math.isnan(want)) or got == want
    # the same run with the option off: bit-identical chains and displacement moments, and no covariance anything
    monkeypatch.setattr(DisplacementCovariance, 'record', record)
    torch.manual_seed(0)
    off = make_trainer(tmp_path / 'off', (N, N, N), **kw)
    off.run()
    assert torch.equal(off.v_curr_state, t.v_curr_state)
    assert torch.equal(off.displacement_mean, t.displacement_mean) and torch.equal(off.displacement_std, t.displacement_std)
    assert off.displacement_cov_std is None and off.displacement_cov_direction is None and off.displacement_cov_anisotropy is None
    assert off.displacement_cov_summary is None and off._displacement_covariance is None
    on_keys, off_keys = list(res), list(off.metrics.result())
    assert not [k for k in off_keys if k.startswith('MCMC/covariance/')]
    assert [k for k in on_keys if not k.startswith('MCMC/covariance/')] == off_keys
    assert [k for k in on_keys if k.startswith('MCMC/covariance/')] == [f'MCMC/covariance/{k}' for k in COVARIANCE_METRICS]
    names = lambda tr: sorted(p.name for p in tr.config.save_dirs['samples'].iterdir())
    assert names(t) == sorted(names(off) + NEW_FILES)


def test_trainer_displacement_covariance_survives_checkpoint_resume_bit_for_bit(tmp_path):
    kw = dict(no_chains=2, no_iters_burn_in=2, no_samples_MCMC=8, log_period_MCMC=4, checkpoint_period=6,
              displacement_covariance={'period': 2}, save_outputs=False)
    a = make_trainer(tmp_path / 'a', (16, 16, 16), **kw)
    a.run()
    ck = a.config.save_dirs['checkpoints'] / 'checkpoint_0000006.pt'
    sd = torch.load(ck, map_location='cpu', weights_only=True)
    assert sd['displacement_covariance']['records'] == 2 * a.no_chains
    assert tuple(sd['displacement_covariance']['comoment'].shape) == (6, 16, 16, 16)
    b = make_trainer(tmp_path / 'b', (16, 16, 16), resume=str(ck), **kw)
    b.run()
    for name in ('displacement_cov_std', 'displacement_cov_direction', 'displacement_cov_anisotropy'):
        assert torch.equal(getattr(a, name).view(torch.int32), getattr(b, name).view(torch.int32)), name
    for name in ('mean', 'comoment'):
        assert torch.equal(getattr(a._displacement_covariance, name), getattr(b._displacement_covariance, name)), name
    assert json.dumps(a.displacement_cov_summary, sort_keys=True) == json.dumps(b.displacement_cov_summary, sort_keys=True)
    # a checkpoint of other dims is refused; one without the key, once a recorded step has passed, too
    with pytest.raises(ValueError, match='shape'):
        DisplacementCovariance((16, 16, 17), DEV).load_state_dict(sd['displacement_covariance'])
    del sd['displacement_covariance']
    ck2 = tmp_path / 'no_covariance.pt'
    torch.save(sd, ck2)
    c = make_trainer(tmp_path / 'c', (16, 16, 16), resume=str(ck2), **kw)
    with pytest.raises(ValueError, match='displacement_covariance'):
        c.run()
    off_kw = {k: v for k, v in kw.items() if k != 'displacement_covariance'}
    off = make_trainer(tmp_path / 'off', (16, 16, 16), **off_kw)
    off.run()
    sd_off = torch.load(off.config.save_dirs['checkpoints'] / 'checkpoint_0000006.pt', map_location='cpu', weights_only=True)
    assert set(sd_off) == set(sd)
