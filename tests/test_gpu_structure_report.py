"""Structure report on the device: the exact known answer, random cases against the numpy restatement with derived tolerances
(tests/_structure_report.py), the map statistics, the empty-structure identities, both stages of the reduction past one round,
determinism, agreement with the Jacobian posterior's fold count, the recorder against the functional form and across a restart
of its state, the ABI and Python refusals, and the trainer option end to end (summary against the recorded samples, coherence
against the recorded covariance state, files, metrics, checkpoint / resume, and nothing changed when it is off)."""
import copy
import ctypes as C
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

from ir_sgmcmc_amd import _lib as L
from ir_sgmcmc_amd import structure_report as sr
from ir_sgmcmc_amd.diagnostics import JacobianPosterior, StructureReport, recorded_steps
from ir_sgmcmc_amd.parse_config import ConfigParser
from ir_sgmcmc_amd.trainer import Trainer
from ir_sgmcmc_amd.utils import calc_structure_report
from tests._jacobian_posterior import CASES, DELTA, RECIPES, case_seed, draw_records, jacobian_posterior_np
from tests._structure_report import (LABEL_RECIPES, covariance_trace_np, label_values, label_volume, map_errors, map_stats_np,
                                     motion_errors, motion_np, summary_np)
from tests.test_structure_report_host import HAND, hand_case

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_motion(u, t, seg, labels, scale=(1.0, 1.0, 1.0), mask=None):
    ints, floats = sr.structure_motion(dev(u), dev(t), dev(seg), labels, scale, None if mask is None else dev(mask))
    return ints.cpu().numpy(), floats.cpu().numpy()


def run_maps(maps, seg, labels, mask=None):
    ints, floats = sr.structure_map_stats(dev(maps), dev(seg), labels, None if mask is None else dev(mask))
    return ints.cpu().numpy(), floats.cpu().numpy()


def test_exact_known_answer():
    """dims (5,9,17): the identity is exact in float32, det = 1.25 exactly, the scaled displacements have integer norms: every
    column is exact in any order"""
    shape, seg, t, u, labels, scale = hand_case()
    ints, floats = run_motion(u, t, seg, labels, scale)
    assert ints.shape == (1, 2, 2) and floats.shape == (1, 2, 9) and ints.dtype == np.int64 and floats.dtype == np.float64
    for j, lab in enumerate(labels):
        w, n2, n1, vox = HAND[lab]
        assert ints[0, j].tolist() == [vox, 0]
        assert floats[0, j].tolist() == [vox * w[0], vox * w[1], vox * w[2], vox * n1, vox * n2, n1, 1.25 * vox, 1.25, 1.25]
    # a folded structure: x mirrored, det = -1.25 exactly
    t2 = t.copy()
    t2[:, 0] *= -1.0
    ints, floats = run_motion(u, t2, seg, labels, scale)
    assert ints[0].tolist() == [[306, 306], [153, 153]] and floats[0, :, 6:].tolist() == [[-1.25 * 306, -1.25, -1.25],
                                                                                          [-1.25 * 153, -1.25, -1.25]]


@functools.lru_cache(maxsize=None)
def case_reference(Cn, steps, shape, recipe):
    """the records of a case, a displacement per record, and the float64 det and its bound: computed once per case"""
    records = draw_records(recipe, Cn * steps, shape, case_seed(Cn, steps, shape, recipe))
    ref = jacobian_posterior_np(records)
    rng = np.random.default_rng(case_seed(Cn, steps, shape, recipe) + 1)
    u = (rng.normal(size=records.shape) * 3.0).astype(np.float32)
    return records, u, ref


@pytest.mark.parametrize('with_mask', [False, True])
@pytest.mark.parametrize('K', [1, 3, 64])
@pytest.mark.parametrize('label_recipe', LABEL_RECIPES)
@pytest.mark.parametrize('recipe', RECIPES)
@pytest.mark.parametrize('Cn,steps,shape', CASES)
def test_random_cases_match_the_restatement(Cn, steps, shape, recipe, label_recipe, K, with_mask):
    records, u, ref = case_reference(Cn, steps, shape, recipe)
    # conditions on the inputs
    assert (np.abs(ref['det']) < DELTA).mean() <= 0.005
    per_record = ref['det'].reshape(len(records), -1)
    assert (ref['e'].reshape(len(records), -1).sum(axis=1) <= 1e-5 * np.abs(per_record).sum(axis=1)).all()
    labels = label_values(K)
    seg = label_volume(label_recipe, shape, labels, shape[2] + K)
    mask = (np.random.default_rng(shape[2]).random(shape) < 0.6) if with_mask else None
    scale = (0.5, 1.0, 2.0)
    worst = 0.0
    for s in range(steps):
        rows = slice(s * Cn, (s + 1) * Cn)
        want = motion_np(u[rows], records[rows], seg, labels, scale, mask,
                         ref={'det': ref['det'][rows], 'e': ref['e'][rows]})
        ints, floats = run_motion(u[rows], records[rows], seg, labels, scale, mask)
        ratio, bad = motion_errors(ints, floats, want)
        worst = max(worst, ratio)
        print({'step': s, 'largest error / tolerance': ratio, 'violations': bad})  # before the assertion
        assert not bad, bad
        empty = want['ints'][..., 0] == 0
        assert (ints[empty] == 0).all() and (floats[empty][:, (0, 1, 2, 3, 4, 6)] == 0).all()
        assert (floats[empty][:, (5, 8)] == -np.inf).all() and (floats[empty][:, 7] == np.inf).all()
    assert worst <= 1.0


@pytest.mark.parametrize('with_mask', [False, True])
@pytest.mark.parametrize('label_recipe', LABEL_RECIPES)
@pytest.mark.parametrize('M,shape,K', [(1, (3, 4, 5), 3), (5, (9, 6, 70), 3), (5, (17, 16, 33), 64), (1, (1, 1, 7), 1)])
def test_map_statistics(M, shape, K, label_recipe, with_mask):
    rng = np.random.default_rng(M * 100 + shape[2])
    maps = (rng.normal(size=(M,) + shape) * 10.0 ** rng.integers(-3, 4, size=(M, 1, 1, 1))).astype(np.float32)
    flat = maps.reshape(-1)
    for value in (np.nan, np.inf, -np.inf):
        flat[rng.integers(flat.size, size=max(flat.size // 50, 1))] = value
    labels = label_values(K)
    seg = label_volume(label_recipe, shape, labels, shape[2] + K)
    mask = (rng.random(shape) < 0.6) if with_mask else None
    want = map_stats_np(maps, seg, labels, mask)
    ints, floats = run_maps(maps, seg, labels, mask)
    ratio, bad = map_errors(ints, floats, want)
    print({'largest error / tolerance': ratio, 'violations': bad})
    assert not bad and ratio <= 1.0


def test_empty_structure_unlisted_volume_and_false_mask():
    shape = (4, 5, 6)
    records = draw_records('smooth', 2, shape, 3)
    u = np.random.default_rng(0).normal(size=records.shape).astype(np.float32)
    identity = ([0, 0], [0.0, 0.0, 0.0, 0.0, 0.0, -math.inf, 0.0, math.inf, -math.inf])
    labels = [3, 4]
    seg = np.full(shape, 3, dtype=np.int16)
    ints, floats = run_motion(u, records, seg, labels)
    assert ints[:, 0, 0].tolist() == [120, 120] and [ints[0, 1].tolist(), floats[0, 1].tolist()] == list(identity)
    for seg_, mask in ((np.full(shape, 7, dtype=np.int16), None), (np.zeros(shape, dtype=np.int16), None),
                       (np.full(shape, -3, dtype=np.int16), None), (seg, np.zeros(shape, dtype=bool))):
        ints, floats = run_motion(u, records, seg_, labels, mask=mask)
        mi, mf = run_maps(u[0], seg_, labels, mask)
        for c in range(2):
            for j in range(2):
                assert [ints[c, j].tolist(), floats[c, j].tolist()] == list(identity)
        assert (mi == 0).all() and mf.tolist() == [[[0.0, 0.0, math.inf, -math.inf]] * 2] * 3
    # a non-finite displacement propagates into its structure's sums and into no other's; a NaN det is folded and left out
    seg[2:] = 4
    u2, t2 = u.copy(), records.copy()
    u2[0, 1, 0, 0, 0] = np.nan
    u2[1, 2, 3, 4, 5] = np.inf
    t2[1, 0, 3, 2, 2] = np.nan
    ints, floats = run_motion(u2, t2, seg, labels)
    assert np.isnan(floats[0, 0, 1]) and np.isnan(floats[0, 0, 3]) and np.isfinite(floats[0, 0, (0, 2, 5, 6)]).all()
    assert np.isfinite(floats[0, 1]).all() and np.isfinite(floats[1, 0]).all()
    assert floats[1, 1, 2] == np.inf and floats[1, 1, 5] == np.inf and np.isfinite(floats[1, 1, 6:]).all()
    want = motion_np(u, t2, seg, labels)
    assert ints[1, 1, 1] >= 1 and want['fold_lo'][1, 1] <= ints[1, 1, 1] <= want['fold_hi'][1, 1]
    assert abs(floats[1, 1, 6] - want['floats'][1, 1, 6]) <= 60 * 2.0 ** -53 * want['abs'][1, 1, 6] + 2 * want['e_sum'][1, 1]


# 263 blocks of partials per row: threads 0 .. 6 of the second stage (256 threads) fold two blocks each, and V % 256 != 0;
# 270 400 voxels: more than the 1024 blocks x 256 threads of a row's grid, so the first stage's grid-stride loop wraps, with a
# ragged tail.  The smallest shapes on either path of this implementation (structure_device.h: kStructureMaxBlocks).
@pytest.mark.parametrize('shape', [(41, 40, 41), (65, 64, 65)])
def test_reduction_past_one_round_of_either_stage(shape):
    records = draw_records('folding', 2, shape, case_seed(2, 1, shape, 'folding'))
    u = (np.random.default_rng(shape[0]).normal(size=records.shape) * 2.0).astype(np.float32)
    labels = label_values(3)
    for label_recipe in LABEL_RECIPES:
        seg = label_volume(label_recipe, shape, labels, 5)
        want = motion_np(u, records, seg, labels)
        ratio, bad = motion_errors(*run_motion(u, records, seg, labels), want)
        print({'labels': label_recipe, 'motion: largest error / tolerance': ratio, 'violations': bad})
        assert not bad and ratio <= 1.0 and (want['ints'][..., 0] > 0).all()
        wm = map_stats_np(u[0], seg, labels)
        ratio, bad = map_errors(*run_maps(u[0], seg, labels), wm)
        print({'labels': label_recipe, 'maps: largest error / tolerance': ratio, 'violations': bad})
        assert not bad and ratio <= 1.0


def test_two_identical_calls_are_bit_identical():
    shape, Cn, K = (37, 41, 43), 3, 64
    records = dev(draw_records('folding', Cn, shape, 11))
    u = dev((np.random.default_rng(1).normal(size=(Cn, 3) + shape) * 2.0).astype(np.float32))
    labels = label_values(K)
    seg = dev(label_volume('white', shape, labels, 2))
    mask = dev(np.random.default_rng(2).random(shape) < 0.7)
    a = sr.structure_motion(u, records, seg, labels, (0.5, 1.0, 2.0), mask)
    b = sr.structure_motion(u, records, seg, labels, (0.5, 1.0, 2.0), mask)
    maps = u.reshape(Cn * 3, *shape)
    c = sr.structure_map_stats(maps, seg, labels, mask)
    d = sr.structure_map_stats(maps, seg, labels, mask)
    for x, y in zip(a + c, b + d):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    assert int(a[0][..., 0].sum()) > 0 and int((a[0][0, :, 0] > 0).sum()) == K


@pytest.mark.parametrize('recipe', RECIPES)
def test_folded_agrees_with_the_jacobian_posterior(recipe):
    shape = (17, 16, 33)
    records = draw_records(recipe, 3, shape, 21)
    records[2, 0] = 0.0  # det == 0 exactly: folded
    t = dev(records)
    seg = torch.full(shape, 5, device=DEV, dtype=torch.int16)
    u = torch.zeros_like(t)
    for r in range(3):
        jp = JacobianPosterior(shape, DEV)
        jp.record(t[r:r + 1].contiguous())
        ints, _ = sr.structure_motion(u[r:r + 1], t[r:r + 1].contiguous(), seg, [5])
        assert ints.cpu().tolist() == [[[shape[0] * shape[1] * shape[2], int(jp.folds.sum())]]]


def test_recorder_equals_the_functional_form_and_survives_a_restart():
    shape = (5, 7, 9)
    n = 11
    t = dev(draw_records('folding', n, shape, 5))
    u = dev((np.random.default_rng(5).normal(size=(n, 3) + shape)).astype(np.float32))
    structures = {'a': 10, 'b': -7, 'nowhere': 4242}
    seg = dev(label_volume('blocks', shape, [10, -7], 1))
    maps = {'first': u[0, 0], 'second': t[3, 1]}
    whole = calc_structure_report(u, t, seg, structures, (1.0, 2.0, 0.5), maps=maps, chains=2)
    assert whole['records'] == n and whole['maps'] == ['first', 'second']
    assert 'first_mean' in whole['structures']['a'] and whole['structures']['nowhere']['second_finite'] == 0

    def feed(report, first, last):
        for i in range(first, last, 2):
            report.record((u[i:min(i + 2, last)].contiguous(), t[i:min(i + 2, last)].contiguous()))

    one = StructureReport(seg, structures, n, DEV)
    feed(one, 0, n)  # five steps of two chains and a last step of one
    assert one.records == n
    for got, want in zip(one.series(), whole['series']):
        assert got.tobytes() == want.tobytes()
    summary, _ = one.finalize((1.0, 2.0, 0.5), 2)
    for name in structures:
        for key in sr.MOTION_KEYS:
            a, b = summary['structures'][name][key], whole['structures'][name][key]
            assert (isinstance(a, float) and math.isnan(a) and math.isnan(b)) or a == b, (name, key)
    # state_dict -> a fresh recorder -> continuing gives the same series
    part = StructureReport(seg, structures, n, DEV)
    feed(part, 0, 6)
    sd = part.state_dict()
    assert sd['records'] == 6 and tuple(sd['ints'].shape) == (n, 3, 2) and tuple(sd['floats'].shape) == (n, 3, 9)
    fresh = StructureReport(seg, structures, n, DEV)
    fresh.load_state_dict(sd)
    feed(fresh, 6, n)
    assert torch.equal(fresh.ints, one.ints) and torch.equal(fresh.floats.view(torch.int64), one.floats.view(torch.int64))
    with pytest.raises(ValueError, match='rows the series was allocated for'):
        fresh.record((u[:1].contiguous(), t[:1].contiguous()))
    with pytest.raises(ValueError, match='does not match this run'):
        StructureReport(seg, structures, n + 1, DEV).load_state_dict(sd)
    with pytest.raises(ValueError, match='structures_dict is empty'):
        StructureReport(seg, {}, n, DEV)
    with pytest.raises(RuntimeError, match='nothing recorded'):
        StructureReport(seg, structures, n, DEV).series()


def test_abi_and_python_refusals():
    lib = L.load()
    Cn, D, H, W, K = 2, 4, 5, 6, 3
    t = dev(draw_records('smooth', Cn, (D, H, W), 1))
    u = torch.ones_like(t)
    seg = torch.full((D, H, W), 10, device=DEV, dtype=torch.int16)
    ints = torch.full((Cn, K, 2), -5, device=DEV, dtype=torch.int64)
    floats = torch.full((Cn, K, 9), -5.0, device=DEV, dtype=torch.float64)
    mints = torch.full((Cn * 3, K, 2), -5, device=DEV, dtype=torch.int64)
    mfloats = torch.full((Cn * 3, K, 4), -5.0, device=DEV, dtype=torch.float64)
    nb = C.c_size_t()
    L.check(lib.irs_structure_workspace(D, H, W, K, Cn * 3, C.byref(nb)))
    assert nb.value == 8 * 11 * Cn * 3 * K * 1  # one block of partials per (row, structure): 120 voxels
    ws = torch.empty(nb.value, device=DEV, dtype=torch.uint8)
    q = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    st = L.stream_ptr()
    lab = lambda *v: (C.c_int32 * max(len(v), 1))(*v)
    good_labels, scale = lab(10, 11, 12), (C.c_float * 3)(1.0, 1.0, 1.0)

    def motion(u_=u, t_=t, C_=Cn, D_=D, seg_=seg, labels=good_labels, K_=K, scale_=scale, ints_=ints, floats_=floats, ws_=ws,
               ws_bytes=nb.value):
        return lib.irs_structure_motion(q(u_), q(t_), C_, D_, H, W, q(seg_), labels, K_, None, scale_, q(ints_), q(floats_), q(ws_),
                                        ws_bytes, st)

    def stats(maps=u, M=Cn * 3, D_=D, seg_=seg, labels=good_labels, K_=K, ints_=mints, floats_=mfloats, ws_=ws, ws_bytes=nb.value):
        return lib.irs_structure_map_stats(q(maps), M, D_, H, W, q(seg_), labels, K_, None, q(ints_), q(floats_), q(ws_), ws_bytes, st)

    for kw in (dict(u_=None), dict(t_=None), dict(seg_=None), dict(labels=None), dict(scale_=None), dict(ints_=None),
               dict(floats_=None), dict(ws_=None), dict(C_=0), dict(C_=9), dict(K_=0), dict(K_=65), dict(labels=lab(10, 11, 10)),
               dict(labels=lab(10, 11, 32768)), dict(labels=lab(10, -32769, 12)), dict(D_=1), dict(D_=0), dict(ws_bytes=nb.value // 3 - 8),
               dict(scale_=(C.c_float * 3)(1.0, 0.0, 1.0)), dict(scale_=(C.c_float * 3)(1.0, float('nan'), 1.0))):
        with pytest.raises(L.IrsError):
            L.check(motion(**kw))
    for kw in (dict(maps=None), dict(seg_=None), dict(labels=None), dict(ints_=None), dict(floats_=None), dict(ws_=None), dict(M=0),
               dict(M=-1), dict(K_=0), dict(K_=65), dict(labels=lab(10, 10, 12)), dict(labels=lab(40000, 11, 12)), dict(D_=0),
               dict(ws_bytes=nb.value - 8)):
        with pytest.raises(L.IrsError):
            L.check(stats(**kw))
    for kw in (dict(D_=0), dict(K_=0), dict(K_=65), dict(rows=0), dict(out=None)):
        a = dict(D_=D, K_=K, rows=2, out=C.byref(nb))
        a.update(kw)
        with pytest.raises(L.IrsError):
            L.check(lib.irs_structure_workspace(a['D_'], H, W, a['K_'], a['rows'], a['out']))
    torch.cuda.synchronize()
    for x in (ints, floats, mints, mfloats):  # a refused call writes nothing
        assert bool((x == -5).all())
    L.check(stats(D_=1, maps=u[:, :, :1].contiguous(), seg_=seg[:1].contiguous()))  # a dim of 1 is fine for the maps
    L.check(motion())
    L.check(stats())
    torch.cuda.synchronize()
    assert ints[:, 0, 0].tolist() == [D * H * W] * Cn and mints[:, 0, 0].tolist() == [D * H * W] * (Cn * 3)
    assert int(ints[:, 1:].sum()) == 0
    # the Python surface checks dtypes, shapes and devices before it calls
    labels = [10, 11, 12]
    for bad in (lambda: sr.structure_motion(u.double(), t, seg, labels),
                lambda: sr.structure_motion(u, t.double(), seg, labels),
                lambda: sr.structure_motion(u.cpu(), t.cpu(), seg.cpu(), labels),
                lambda: sr.structure_motion(u, t[:1].contiguous(), seg, labels),
                lambda: sr.structure_motion(u[:, :2].contiguous(), t, seg, labels),
                lambda: sr.structure_motion(u, t, seg.int(), labels),
                lambda: sr.structure_motion(u, t, seg[:2].contiguous(), labels),
                lambda: sr.structure_motion(u, t, seg, labels, scale=(1.0, 2.0)),
                lambda: sr.structure_motion(u, t, seg, labels, scale=(1.0, -2.0, 1.0)),
                lambda: sr.structure_motion(u, t, seg, []),
                lambda: sr.structure_motion(u, t, seg, [1, 1]),
                lambda: sr.structure_motion(u, t, seg, labels, mask=torch.ones(D, H, W, device=DEV)),
                lambda: sr.structure_motion(u, t, seg, labels, mask=torch.ones(D, H, W + 1, device=DEV, dtype=torch.bool)),
                lambda: sr.structure_motion(u, t, seg, labels, out=(ints.int(), floats)),
                lambda: sr.structure_motion(u, t, seg, labels, out=(ints, floats[:, :2])),
                lambda: sr.structure_motion(u, t, seg, labels, out=(ints.cpu(), floats.cpu())),
                lambda: sr.structure_map_stats(u, seg, labels),
                lambda: sr.structure_map_stats(u[0].double(), seg, labels),
                lambda: sr.structure_map_stats(u[0].cpu(), seg.cpu(), labels),
                lambda: sr.structure_map_stats(u[0], seg.float(), labels),
                lambda: sr.structure_map_stats(u[0], seg, list(range(65)))):
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


def test_trainer_end_to_end(tmp_path, monkeypatch):
    N = 24
    kept = []
    record = StructureReport.record

    def spy(self, sample):
        kept.append(tuple(x.clone() for x in sample))
        return record(self, sample)

    monkeypatch.setattr(StructureReport, 'record', spy)
    kw = dict(no_chains=2, no_iters_burn_in=3, no_samples_MCMC=9, log_period_MCMC=4)
    torch.manual_seed(0)
    t = make_trainer(tmp_path / 'on', (N, N, N), structure_report={'period': 2}, displacement_covariance={'period': 2}, **kw)
    t.run()
    Cn = t.no_chains
    steps = recorded_steps(3, 9, 2)
    assert Cn == 2 and len(kept) == len(steps) == 4 and t._structure_report.records == 8
    u = torch.cat([k[0] for k in kept]).cpu().numpy()
    tr = torch.cat([k[1] for k in kept]).cpu().numpy()
    names, labels = list(t.structures_dict), list(t.structures_dict.values())
    seg = next(iter(t.data_loader))[0]['seg'].reshape(N, N, N).numpy()
    s = t.structure_summary
    assert s['records'] == 8 and list(s['structures']) == names
    # the device series against the restatement of the kept samples, then the summary against the restatement of the series
    ints, floats = t._structure_report.series()
    want = motion_np(u, tr, seg, labels)
    ratio, bad = motion_errors(ints, floats, want)
    print({'largest error / tolerance': ratio, 'violations': bad})
    assert not bad and ratio <= 1.0
    comoment = t._displacement_covariance.comoment[:3].cpu().numpy()
    assert t._displacement_covariance.records == 8
    ms = map_stats_np(comoment, seg, labels)
    trace = sr.covariance_trace(ms['ints'], ms['floats'], 8)
    table = summary_np(ints, floats, names, spacing=[float(x) for x in t.data_loader.im_spacing] if
                       getattr(t.data_loader, 'im_spacing', None) is not None else (1.0, 1.0, 1.0), chains=Cn, cov_trace=trace)
    present = [n for n in names if s['structures'][n]['voxels'] > 0]
    assert present and len(present) < len(names)  # the synthetic segmentation carries some of the structures: both kinds of row
    keys = sr.MOTION_KEYS + sr.COHERENCE_KEYS
    for name in names:
        row = s['structures'][name]
        assert list(row)[:len(keys)] == list(keys)
        for key in keys:
            assert row[key] == pytest.approx(table[name][key], rel=1e-9, abs=1e-12, nan_ok=True), (name, key)
    # coherence: against the float64 covariance of the kept displacements, and <= 1 up to the float32 co-moments
    exact = covariance_trace_np(u, seg, labels)
    for j, name in enumerate(names):
        row = s['structures'][name]
        if row['voxels'] > 0:
            assert row['coherence'] <= 1.0 + 1e-4 and row['coherence'] > 0
            assert trace[j] == pytest.approx(exact[j], rel=1e-3)
            assert row['rhat_max'] >= 0.0 or math.isnan(row['rhat_max'])  # 4 records per chain
    # the map rows: every finished map, by its own restatement
    assert s['maps'] == ['displacement_std_x', 'displacement_std_y', 'displacement_std_z', 'displacement_std_norm',
                         'displacement_cov_std_major', 'displacement_cov_anisotropy']
    std = t.displacement_std.cpu().numpy()
    wm = map_stats_np(std, seg, labels)
    rows = sr.structure_map_rows(wm['ints'], wm['floats'], s['maps'][:3], names)
    for name in present:
        for key, v in rows[name].items():
            assert s['structures'][name][key] == pytest.approx(v, rel=1e-7, nan_ok=True), (name, key)
    # files
    folder = t.config.save_dirs['samples']
    header, lines = sr.read_csv(folder / 'MCMC_structures.csv')
    assert header == ['structure'] + list(s['structures'][names[0]]) and [line[0] for line in lines] == names
    for line in lines:
        for key, cell in zip(header[1:], line[1:]):
            w = s['structures'][line[0]][key]
            assert (isinstance(cell, float) and math.isnan(cell) and math.isnan(w)) or cell == w, (line[0], key)
    sheader, slines = sr.read_csv(folder / 'MCMC_structure_series.csv')
    assert tuple(sheader) == sr.SERIES_COLUMNS and len(slines) == 8 * len(names)
    assert [line[1] for line in slines[::len(names)]] == [st for st in steps for _ in range(Cn)]
    j = names.index(present[0])
    line = slines[3 * len(names) + j]
    assert line[:4] == [3, steps[1], 1, present[0]] and line[4] == floats[3, j, 0] / ints[3, j, 0] and line[9] == ints[3, j, 1]
    # metrics
    res = t.metrics.result()
    for name in names:
        for key in keys:
            got, w = res[f'MCMC/structure/{key}/{name}'], s['structures'][name][key]
            assert (math.isnan(got) and math.isnan(w)) or got == w
    # the same run with the option off: bit-identical chains and moments, and no structure anything
    monkeypatch.setattr(StructureReport, 'record', record)
    torch.manual_seed(0)
    off = make_trainer(tmp_path / 'off', (N, N, N), displacement_covariance={'period': 2}, **kw)
    off.run()
    assert torch.equal(off.v_curr_state, t.v_curr_state)
    assert torch.equal(off.displacement_mean, t.displacement_mean) and torch.equal(off.displacement_std, t.displacement_std)
    assert off.structure_summary is None and off._structure_report is None
    on_keys, off_keys = list(res), list(off.metrics.result())
    assert not [k for k in off_keys if k.startswith('MCMC/structure/')]
    assert [k for k in on_keys if not k.startswith('MCMC/structure/')] == off_keys
    listing = lambda tr_: sorted(p.name for p in tr_.config.save_dirs['samples'].iterdir())
    assert listing(t) == sorted(listing(off) + ['MCMC_structures.csv', 'MCMC_structure_series.csv'])


def test_trainer_checkpoint_resume_gives_the_same_files(tmp_path):
    kw = dict(no_chains=2, no_iters_burn_in=2, no_samples_MCMC=8, log_period_MCMC=4, checkpoint_period=6,
              structure_report={'period': 2, 'maps': True}, displacement_covariance={'period': 2})
    a = make_trainer(tmp_path / 'a', (16, 16, 16), **kw)
    a.run()
    ck = a.config.save_dirs['checkpoints'] / 'checkpoint_0000006.pt'
    sd = torch.load(ck, map_location='cpu', weights_only=True)
    K = len(a.structures_dict)
    assert sd['structure_report']['records'] == 2 * a.no_chains
    assert tuple(sd['structure_report']['ints'].shape) == (8, K, 2) and tuple(sd['structure_report']['floats'].shape) == (8, K, 9)
    b = make_trainer(tmp_path / 'b', (16, 16, 16), resume=str(ck), **kw)
    b.run()
    for name in ('MCMC_structures.csv', 'MCMC_structure_series.csv'):
        fa, fb = (x.config.save_dirs['samples'] / name for x in (a, b))
        assert fa.read_bytes() == fb.read_bytes() and fa.stat().st_size > 0, name
    assert json.dumps(a.structure_summary, sort_keys=True) == json.dumps(b.structure_summary, sort_keys=True)
    # a checkpoint without the key, once a recorded step has passed, is refused; with the option off the key does not exist
    del sd['structure_report']
    ck2 = tmp_path / 'no_structures.pt'
    torch.save(sd, ck2)
    c = make_trainer(tmp_path / 'c', (16, 16, 16), resume=str(ck2), **kw)
    with pytest.raises(ValueError, match='structure_report'):
        c.run()
    off_kw = {k: v for k, v in kw.items() if k != 'structure_report'}
    off = make_trainer(tmp_path / 'off', (16, 16, 16), save_outputs=False, **off_kw)
    off.run()
    sd_off = torch.load(off.config.save_dirs['checkpoints'] / 'checkpoint_0000006.pt', map_location='cpu', weights_only=True)
    assert set(sd_off) == set(sd)
