"""Jacobian posterior on the device: the known answer and random cases against the numpy restatement, the summary reduction,
determinism, agreement with the per-sample fold count, the ABI and Python refusals, and the trainer option end to end (maps
against the recorded transformations, files, metrics, checkpoint / resume, and nothing changed when it is off).

Fold counts are compared at every voxel: with DELTA = 1e-3, #(det64 <= -DELTA) <= folds <= #(det64 < DELTA).  Moments and maps
are compared at every voxel none of whose records has |det64| < DELTA, against the tolerances of tests/_jacobian_posterior.py
(the propagated rounding bound of det plus the float32 Welford terms, times FACTOR = 2); test_jacobian_posterior_host.py checks
on the CPU that a float32 evaluation of the same inputs stays inside them."""
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
from ir_sgmcmc_amd.diagnostics import JACOBIAN_METRICS, JacobianPosterior, recorded_steps
from ir_sgmcmc_amd.parse_config import ConfigParser
from ir_sgmcmc_amd.trainer import Trainer
from ir_sgmcmc_amd.utils import calc_jacobian_posterior
from tests._jacobian_posterior import (CASES, DELTA, RECIPES, case_seed, draw_records, fold_bounds, jacobian_posterior_np, maps_np,
                                       summary_np, tolerances)
from tests.test_jacobian_posterior_host import HAND_MEAN, HAND_STD, hand_checked_records

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_KEYS = ('records', 'voxels', 'folded_voxels', 'always_folded', 'fold_records')
FLOAT_KEYS = ('fold_prob_max', 'fold_prob_mean', 'logJ_mean_min', 'logJ_mean_max', 'logJ_std_mean', 'logJ_std_max')


def run_device(records, C, mask=None):
    """records (n,3,D,H,W) float32 in record order, C chains per step -> (JacobianPosterior, the three maps as numpy, summary)"""
    n = records.shape[0]
    assert n % C == 0
    jp = JacobianPosterior(records.shape[2:], DEV)
    rec = torch.from_numpy(records).to(DEV)
    for s in range(n // C):
        jp.record(rec[s * C:(s + 1) * C].contiguous())
    m = None if mask is None else torch.from_numpy(mask).to(DEV)
    fp, lm, ls, summary = jp.finalize(m)
    return jp, fp.cpu().numpy(), lm.cpu().numpy(), ls.cpu().numpy(), summary


def check_against_restatement(jp, fp, lm, ls, summary, ref, mask=None, max_band=0.005):
    n = ref['n']
    folds = jp.folds.cpu().numpy()
    mean, m2 = jp.mean.cpu().numpy(), jp.m2.cpu().numpy()
    band = np.abs(ref['det']) < DELTA
    assert band.mean() <= max_band, band.mean()  # a condition on the inputs
    lo, hi = fold_bounds(ref['det'])
    assert ((lo <= folds) & (folds <= hi)).all()  # no voxel left out
    clear, tol_mean, tol_root, tol_std = tolerances(ref)
    assert np.array_equal(folds[clear], ref['folds'][clear])
    v = clear & (ref['k'] > 0)
    figures = {'voxels compared': int(v.sum()), 'of': int(v.size)}
    for name, got, want, tol in (('mean', mean, ref['mean'], tol_mean),
                                 ('sqrt m2', np.sqrt(m2.astype(np.float64)), np.sqrt(ref['m2']), tol_root),
                                 ('logJ_std', ls, ref['logJ_std'], tol_std)):
        err = np.abs(got.astype(np.float64) - want)[v]
        figures[name] = (float(err.max()) if err.size else 0.0, float((err / np.maximum(tol[v], 1e-300)).max()) if err.size else 0.0)
    print(figures)  # largest error and largest error / tolerance, before the assertions
    for name in ('mean', 'sqrt m2', 'logJ_std'):
        assert figures[name][1] <= 1.0, (name, figures[name])
    # the maps are the state's: fold_prob = float32(folds / n), logJ_mean = mean, NaN where no record is valid
    k = n - folds.astype(np.int64)
    assert np.array_equal(fp, (folds.astype(np.float64) / n).astype(np.float32))
    assert np.array_equal(lm[k >= 1], mean[k >= 1]) and np.isnan(lm[k < 1]).all() and np.isnan(ls[k < 1]).all()
    want_std = np.sqrt(m2[k >= 1].astype(np.float64) / np.maximum(k[k >= 1] - 1, 1))
    assert (np.abs(ls[k >= 1] - want_std) <= 2.0 ** -22 * want_std).all()  # a float32 division and a square root
    # the summary: integers exactly, floats against the restatement of the DEVICE's stored maps (this pins the reduction)
    want = summary_np(folds, n, fp, lm, ls, mask)
    for key in INT_KEYS:
        assert summary[key] == want[key], (key, summary[key], want[key])
    for key in FLOAT_KEYS:
        g, w = summary[key], want[key]
        assert (math.isnan(g) and math.isnan(w)) or abs(g - w) <= 1e-6 * abs(w), (key, g, w)


def test_known_answer():
    records = hand_checked_records()
    jp, fp, lm, ls, s = run_device(records, 2)
    assert jp.records == 4
    assert (jp.folds.cpu().numpy() == 1).all() and (fp == 0.25).all()
    assert np.abs(lm - HAND_MEAN).max() <= 1e-5 and np.abs(ls - HAND_STD).max() <= 1e-5
    assert (s['voxels'], s['folded_voxels'], s['always_folded'], s['fold_records']) == (60, 60, 0, 60)
    assert s['fold_prob_max'] == 0.25 and s['fold_prob_mean'] == 0.25
    assert s['logJ_std_mean'] == pytest.approx(HAND_STD, abs=1e-5) and s['logJ_mean_min'] == pytest.approx(HAND_MEAN, abs=1e-5)
    check_against_restatement(jp, fp, lm, ls, s, jacobian_posterior_np(records))


@pytest.mark.parametrize('with_mask', [False, True])
@pytest.mark.parametrize('recipe', RECIPES)
@pytest.mark.parametrize('C,steps,shape', CASES)
def test_random_cases_match_the_restatement(C, steps, shape, recipe, with_mask):
    records = draw_records(recipe, C * steps, shape, case_seed(C, steps, shape, recipe))
    mask = (np.random.default_rng(shape[2]).random(shape) < 0.6) if with_mask else None
    jp, fp, lm, ls, s = run_device(records, C, mask)
    assert jp.records == C * steps
    check_against_restatement(jp, fp, lm, ls, s, jacobian_posterior_np(records, mask), mask)


def test_folded_everywhere_nan_inputs_and_an_empty_mask():
    shape = (4, 5, 6)
    records = draw_records('smooth', 4, shape, 3)
    records[:, 0] = 0.0  # x collapsed: det == 0 exactly in every record
    jp, fp, lm, ls, s = run_device(records, 2)
    assert (fp == 1).all() and np.isnan(lm).all() and np.isnan(ls).all()
    assert s['always_folded'] == s['voxels'] == 120 and s['fold_prob_max'] == 1.0 and s['fold_prob_mean'] == 1.0
    assert all(math.isnan(s[k]) for k in ('logJ_mean_min', 'logJ_mean_max', 'logJ_std_mean', 'logJ_std_max'))
    records = draw_records('smooth', 2, shape, 4)
    records[1, 2, 1, 2, 3] = np.nan
    ref = jacobian_posterior_np(records)
    jp, fp, lm, ls, s = run_device(records, 2)
    assert np.isnan(ref['det'][1]).sum() >= 1 and (jp.folds.cpu().numpy()[np.isnan(ref['det'][1])] >= 1).all()
    check_against_restatement(jp, fp, lm, ls, s, ref, max_band=1.0)
    _, _, _, _, s0 = run_device(records, 2, np.zeros(shape, dtype=bool))
    assert s0['voxels'] == 0 and all(math.isnan(s0[k]) for k in FLOAT_KEYS)


def test_functional_form_and_restart_of_the_state():
    records = draw_records('folding', 11, (5, 7, 9), 5)  # more records than one launch folds
    t = torch.from_numpy(records).to(DEV)
    fp, lm, ls, s = calc_jacobian_posterior(t)
    ref = jacobian_posterior_np(records)
    lo, hi = fold_bounds(ref['det'])
    assert s['records'] == 11 and int(lo.sum()) <= s['fold_records'] <= int(hi.sum())
    jp = JacobianPosterior((5, 7, 9), DEV)
    jp.folds.fill_(7)  # records_before = 0 overwrites whatever the state held
    jp.mean.fill_(3.0)
    jp.m2.fill_(float('nan'))
    jp.record(t[:8].contiguous())
    jp.record(t[8:].contiguous())
    out = jp.finalize()
    for got, want in zip(out[:3], (fp, lm, ls)):
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert json.dumps(out[3], sort_keys=True) == json.dumps(s, sort_keys=True)
    valid = (ref['k'] > 0)
    assert np.isfinite(jp.m2.cpu().numpy()[valid]).all()


def test_two_update_sequences_and_two_finalize_calls_are_bit_identical():
    records = draw_records('folding', 6, (37, 41, 43), 11)  # more than one block of partials
    mask = np.random.default_rng(2).random((37, 41, 43)) < 0.3
    a = run_device(records, 3, mask)
    b = run_device(records, 3, mask)
    for x, y in ((a[0].folds, b[0].folds), (a[0].mean, b[0].mean), (a[0].m2, b[0].m2)):
        assert torch.equal(x, y)
    for x, y in zip(a[1:4], b[1:4]):
        assert np.array_equal(x, y, equal_nan=True)
    assert json.dumps(a[4], sort_keys=True) == json.dumps(b[4], sort_keys=True)
    m = torch.from_numpy(mask).to(DEV)
    r1 = ops.jacobian_posterior_finalize(a[0].folds, a[0].mean, a[0].m2, 6, m)
    r2 = ops.jacobian_posterior_finalize(a[0].folds, a[0].mean, a[0].m2, 6, m)
    for u, v in zip(r1, r2):
        assert torch.equal(u.view(torch.uint8), v.view(torch.uint8))
    assert r1[3].dtype == torch.int64 and int(r1[3][0]) == int(mask.sum()) and r1[4].dtype == torch.float64


# 263 blocks of partials: threads 0 .. 6 of the second stage fold two blocks each, and V % 256 != 0; 270 400 voxels: more than
# 1024 blocks x 256, so the first stage's grid-stride loop wraps, with a ragged tail.  The smallest shapes on either path.
@pytest.mark.parametrize('shape', [(41, 40, 41), (65, 64, 65)])
def test_summary_reduction_past_one_round_of_either_stage(shape):
    """the summary against the restatement of the DEVICE's stored maps, as check_against_restatement pins the reduction:
    integers exactly, floats to 1e-6 relative, NaN where the restatement has NaN"""
    records = draw_records('folding', 3, shape, case_seed(3, 1, shape, 'folding'))
    jp = JacobianPosterior(shape, DEV)
    jp.record(torch.from_numpy(records).to(DEV).contiguous())
    folds = jp.folds.cpu().numpy()
    for mask in (np.random.default_rng(shape[2]).random(shape) < 0.6, None):
        fp, lm, ls, summary = jp.finalize(None if mask is None else torch.from_numpy(mask).to(DEV))
        want = summary_np(folds, 3, fp.cpu().numpy(), lm.cpu().numpy(), ls.cpu().numpy(), mask)
        print({key: (summary[key], want[key]) for key in INT_KEYS + FLOAT_KEYS})
        assert 0 < want['folded_voxels'] and want['always_folded'] < want['voxels']  # every column has something to reduce
        for key in INT_KEYS:
            assert summary[key] == want[key], (key, summary[key], want[key])
        for key in FLOAT_KEYS:
            g, w = summary[key], want[key]
            assert (math.isnan(g) and math.isnan(w)) or abs(g - w) <= 1e-6 * abs(w), (key, g, w)


@pytest.mark.parametrize('recipe', RECIPES)
def test_fold_count_agrees_with_the_per_sample_operator(recipe):
    shape = (17, 16, 33)
    records = draw_records(recipe, 3, shape, 21)
    records[2, 0] = 0.0  # det == 0 exactly: log is -inf, which the per-sample NaN count leaves out
    t = torch.from_numpy(records).to(DEV)
    for r in range(3):
        jp = JacobianPosterior(shape, DEV)
        jp.record(t[r:r + 1].contiguous())
        cnt, ld = ops.log_det_jacobian(t[r:r + 1].contiguous())
        neg_inf = int((ld == float('-inf')).sum())
        assert int(jp.folds.sum()) == int(cnt[0]) + neg_inf
        assert neg_inf == (shape[0] * shape[1] * shape[2] if r == 2 else 0)
        # and where the record is valid, the mean IS the operator's log det J
        ok = jp.folds == 0
        assert torch.equal(jp.mean[ok], ld[0][ok])


def test_abi_and_python_refusals():
    lib = L.load()
    Cn, D, H, W = 2, 4, 5, 6
    t = torch.from_numpy(draw_records('smooth', Cn, (D, H, W), 1)).to(DEV)
    folds = torch.zeros(D, H, W, device=DEV, dtype=torch.int32)
    mean = torch.zeros(D, H, W, device=DEV)
    m2 = torch.zeros(D, H, W, device=DEV)
    maps = [torch.empty(D, H, W, device=DEV) for _ in range(3)]
    isum = torch.empty(4, device=DEV, dtype=torch.int64)
    fsum = torch.empty(5, device=DEV, dtype=torch.float64)
    ws = torch.empty(L.IRS_JACOBIAN_WS_BYTES, device=DEV, dtype=torch.uint8)
    q = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    st = L.stream_ptr()

    def upd(t_=t, C_=Cn, D_=D, folds_=folds, mean_=mean, m2_=m2, before=0):
        return lib.irs_jacobian_posterior_update(q(t_), C_, D_, H, W, q(folds_), q(mean_), q(m2_), before, st)

    def fin(folds_=folds, mean_=mean, m2_=m2, D_=D, n=2, fp=maps[0], lm=maps[1], ls=maps[2], isum_=isum, fsum_=fsum, ws_=ws,
            ws_bytes=L.IRS_JACOBIAN_WS_BYTES):
        return lib.irs_jacobian_posterior_finalize(q(folds_), q(mean_), q(m2_), D_, H, W, n, None, q(fp), q(lm), q(ls), q(isum_),
                                                   q(fsum_), q(ws_), ws_bytes, st)

    for kw in (dict(t_=None), dict(folds_=None), dict(mean_=None), dict(m2_=None), dict(C_=0), dict(C_=9), dict(D_=1),
               dict(D_=0), dict(before=-1), dict(before=2 ** 31 - 2)):
        with pytest.raises(L.IrsError):
            L.check(upd(**kw))
    for kw in (dict(folds_=None), dict(mean_=None), dict(m2_=None), dict(fp=None), dict(lm=None), dict(ls=None), dict(isum_=None),
               dict(fsum_=None), dict(ws_=None), dict(D_=1), dict(n=0), dict(n=-1), dict(ws_bytes=8)):
        with pytest.raises(L.IrsError):
            L.check(fin(**kw))
    torch.cuda.synchronize()
    assert int(folds.sum()) == 0 and float(mean.abs().sum()) == 0.0  # nothing was folded in by a refused call
    L.check(upd())
    L.check(fin())
    torch.cuda.synchronize()
    assert isum.cpu().tolist()[0] == D * H * W
    # the Python surface checks dtypes, shapes and devices before it calls
    for bad in (lambda: ops.jacobian_posterior_update(t.double(), folds, mean, m2, 0),
                lambda: ops.jacobian_posterior_update(t.cpu(), folds, mean, m2, 0),
                lambda: ops.jacobian_posterior_update(t[:, :2].contiguous(), folds, mean, m2, 0),
                lambda: ops.jacobian_posterior_update(t[:, :, :2].contiguous(), folds, mean, m2, 0),
                lambda: ops.jacobian_posterior_update(t, folds.long(), mean, m2, 0),
                lambda: ops.jacobian_posterior_update(t, folds, mean.double(), m2, 0),
                lambda: ops.jacobian_posterior_update(t, folds, mean, m2[:, :, :3], 0),
                lambda: ops.jacobian_posterior_update(t, folds.cpu(), mean.cpu(), m2.cpu(), 0),
                lambda: ops.jacobian_posterior_finalize(folds, mean, m2, 0),
                lambda: ops.jacobian_posterior_finalize(folds.cpu(), mean.cpu(), m2.cpu(), 2),
                lambda: ops.jacobian_posterior_finalize(folds.float(), mean, m2, 2),
                lambda: ops.jacobian_posterior_finalize(folds, mean[:2], m2, 2),
                lambda: ops.jacobian_posterior_finalize(folds.reshape(-1), mean.reshape(-1), m2.reshape(-1), 2),
                lambda: ops.jacobian_posterior_finalize(folds, mean, m2, 2, mask=torch.ones(D, H, W + 1, device=DEV, dtype=torch.bool)),
                lambda: ops.jacobian_posterior_finalize(folds, mean, m2, 2, mask=torch.ones(D, H, W, device=DEV))):
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


def test_trainer_maps_match_the_recorded_transformations(tmp_path, monkeypatch):
    from ir_sgmcmc_amd.utils.imageio import read_nifti
    N = 24
    kept = []
    record = JacobianPosterior.record

    def spy(self, transformation):
        kept.append(transformation.clone())
        return record(self, transformation)

    monkeypatch.setattr(JacobianPosterior, 'record', spy)
    kw = dict(no_chains=2, no_iters_burn_in=3, no_samples_MCMC=9, log_period_MCMC=4)
    torch.manual_seed(0)
    t = make_trainer(tmp_path / 'on', (N, N, N), jacobian_posterior={'period': 2}, **kw)
    t.run()
    C = t.no_chains
    assert C == 2 and len(kept) == len(recorded_steps(3, 9, 2)) == 9 // 2 and t._jacobian_posterior.records == C * (9 // 2)
    records = torch.cat(kept).cpu().numpy()  # steps in order, chains in order within a step
    mask = next(iter(t.data_loader))[0]['mask'].reshape(N, N, N).numpy() != 0
    ref = jacobian_posterior_np(records, mask)
    fp, lm, ls = (x.cpu().numpy() for x in (t.jacobian_fold_prob, t.jacobian_logJ_mean, t.jacobian_logJ_std))
    check_against_restatement(t._jacobian_posterior, fp, lm, ls, t.jacobian_summary, ref, mask)
    # files
    folder = t.config.save_dirs['samples']
    got, _ = read_nifti(str(folder / 'MCMC_fold_prob.nii.gz'))
    assert np.array_equal(got, fp)
    for name, im in (('logJ_mean', lm), ('logJ_std', ls)):
        plain, _ = read_nifti(str(folder / f'MCMC_{name}.nii.gz'))
        assert np.array_equal(plain, im, equal_nan=True)
        masked, _ = read_nifti(str(folder / f'MCMC_{name}_masked.nii.gz'))
        assert np.array_equal(masked[mask], im[mask], equal_nan=True) and not masked[~mask].any()
    # metrics
    res = t.metrics.result()
    for k in JACOBIAN_METRICS:
        got, want = res[f'MCMC/jacobian/{k}'], t.jacobian_summary[k]
        assert (math.isnan(got) and math.isnan(want)) or got == want
    # the same run with the option off: bit-identical chains and displacement moments, and no Jacobian anything
    monkeypatch.setattr(JacobianPosterior, 'record', record)
    torch.manual_seed(0)
    off = make_trainer(tmp_path / 'off', (N, N, N), **kw)
    off.run()
    assert torch.equal(off.v_curr_state, t.v_curr_state)
    assert torch.equal(off.displacement_mean, t.displacement_mean) and torch.equal(off.displacement_std, t.displacement_std)
    assert off.jacobian_fold_prob is None and off.jacobian_logJ_mean is None and off.jacobian_logJ_std is None
    assert off.jacobian_summary is None and off._jacobian_posterior is None
    on_keys, off_keys = list(res), list(off.metrics.result())
    assert not [k for k in off_keys if k.startswith('MCMC/jacobian/')]
    assert [k for k in on_keys if not k.startswith('MCMC/jacobian/')] == off_keys
    assert [k for k in on_keys if k.startswith('MCMC/jacobian/')] == [f'MCMC/jacobian/{k}' for k in JACOBIAN_METRICS]
    names = lambda tr: sorted(p.name for p in tr.config.save_dirs['samples'].iterdir())
    new_files = ['MCMC_fold_prob.nii.gz', 'MCMC_logJ_mean.nii.gz', 'MCMC_logJ_mean_masked.nii.gz', 'MCMC_logJ_std.nii.gz',
                 'MCMC_logJ_std_masked.nii.gz']
    assert names(t) == sorted(names(off) + new_files)


def test_trainer_jacobian_posterior_survives_checkpoint_resume_bit_for_bit(tmp_path):
    kw = dict(no_chains=2, no_iters_burn_in=2, no_samples_MCMC=8, log_period_MCMC=4, checkpoint_period=6,
              jacobian_posterior={'period': 2}, save_outputs=False)
    a = make_trainer(tmp_path / 'a', (16, 16, 16), **kw)
    a.run()
    ck = a.config.save_dirs['checkpoints'] / 'checkpoint_0000006.pt'
    sd = torch.load(ck, map_location='cpu', weights_only=True)
    assert sd['jacobian_posterior']['records'] == 2 * a.no_chains
    assert tuple(sd['jacobian_posterior']['folds'].shape) == (16, 16, 16)
    b = make_trainer(tmp_path / 'b', (16, 16, 16), resume=str(ck), **kw)
    b.run()
    for name in ('jacobian_fold_prob', 'jacobian_logJ_mean', 'jacobian_logJ_std'):
        assert torch.equal(getattr(a, name).view(torch.int32), getattr(b, name).view(torch.int32)), name
    for name in ('folds', 'mean', 'm2'):
        assert torch.equal(getattr(a._jacobian_posterior, name), getattr(b._jacobian_posterior, name)), name
    assert json.dumps(a.jacobian_summary, sort_keys=True) == json.dumps(b.jacobian_summary, sort_keys=True)
    # a checkpoint of other dims is refused; one without the key, once a recorded step has passed, too
    with pytest.raises(ValueError, match='shape'):
        JacobianPosterior((16, 16, 17), DEV).load_state_dict(sd['jacobian_posterior'])
    del sd['jacobian_posterior']
    ck2 = tmp_path / 'no_jacobian.pt'
    torch.save(sd, ck2)
    c = make_trainer(tmp_path / 'c', (16, 16, 16), resume=str(ck2), **kw)
    with pytest.raises(ValueError, match='jacobian_posterior'):
        c.run()
    off_kw = {k: v for k, v in kw.items() if k != 'jacobian_posterior'}
    off = make_trainer(tmp_path / 'off', (16, 16, 16), **off_kw)
    off.run()
    sd_off = torch.load(off.config.save_dirs['checkpoints'] / 'checkpoint_0000006.pt', map_location='cpu', weights_only=True)
    assert set(sd_off) == set(sd)
