"""Posterior label maps on the device: the known answer and random cases against the numpy restatement, determinism, the ABI
and Python refusals, and the trainer option end to end (maps against the recorded warps, files, metrics, checkpoint /
resume, and nothing changed when it is off)."""
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
from ir_sgmcmc_amd.diagnostics import LabelPosterior, recorded_steps
from ir_sgmcmc_amd.parse_config import ConfigParser
from ir_sgmcmc_amd.trainer import Trainer
from ir_sgmcmc_amd.utils import calc_label_posterior
from tests._label_posterior import BINS, derived_np, label_posterior_np

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LN2 = math.log(2.0)


def run_device(records, C, seg_fixed, structures, mask=None, spacing=(1.0, 1.0, 1.0)):
    """records (n, D, H, W) in record order, C chains per step -> (LabelPosterior, entropy, map, summary)"""
    n = records.shape[0]
    assert n % C == 0
    lp = LabelPosterior(structures, records.shape[1:], DEV)
    rec = torch.from_numpy(records.astype(np.int16)).to(DEV)
    for s in range(n // C):
        lp.record(rec[s * C:(s + 1) * C].unsqueeze(1).contiguous())
    m = None if mask is None else torch.from_numpy(mask).to(DEV)
    e, mp, summary = lp.finalize(torch.from_numpy(seg_fixed.astype(np.int16)), m, spacing)
    return lp, e.cpu().numpy(), mp.cpu().numpy(), summary


def check_against_restatement(lp, e, mp, summary, ref, spacing=(1.0, 1.0, 1.0)):
    assert np.array_equal(lp.counts.cpu().numpy(), ref['counts'])
    assert np.array_equal(mp, ref['map'])
    assert np.abs(e.astype(np.float64) - ref['entropy']).max() <= 1e-6
    assert np.array_equal(summary['raw'], ref['summary'])
    vol = lp.volume.cpu().numpy()
    for got, want in ((vol[:, 0], ref['vol_mean']), (vol[:, 1], ref['vol_m2'])):
        assert np.all(np.abs(got - want) <= 1e-12 * np.maximum(np.abs(want), 1e-300)), (got, want)
    per, ece, e_mean, e_max = derived_np(ref, spacing)
    for name, want in zip(lp.names, per):
        got = summary['structures'][name]
        for k, w in want.items():
            g = got[k]
            assert (math.isnan(g) and math.isnan(w)) or abs(g - w) <= 1e-12 * max(abs(w), 1e-300), (name, k, g, w)
    assert (math.isnan(summary['ECE']) and math.isnan(ece)) or abs(summary['ECE'] - ece) <= 1e-12 * max(ece, 1e-300)
    assert summary['voxels'] == ref['entropy_voxels']
    if ref['entropy_voxels']:
        assert abs(summary['entropy_mean'] - e_mean) <= 1e-6 and abs(summary['entropy_max'] - e_max) <= 1e-6
    else:
        assert math.isnan(summary['entropy_mean']) and math.isnan(summary['entropy_max'])


def test_known_answer():
    records = np.array([[10, 10, 0], [10, 16, 0], [10, 16, 16], [10, 0, 16]]).reshape(4, 1, 1, 3)
    fixed = np.array([10, 16, 0]).reshape(1, 1, 3)
    lp, e, mp, s = run_device(records, 2, fixed, {'A': 10, 'B': 16})
    assert lp.records == 4
    assert lp.counts.cpu().numpy().reshape(2, 3).tolist() == [[4, 1, 0], [0, 2, 2]]
    assert np.abs(e.reshape(-1) - np.array([0.0, 1.5 * LN2, LN2])).max() <= 1e-6 and e.reshape(-1)[0] == 0.0
    assert mp.reshape(-1).tolist() == [10, 16, 0]
    a, b = s['structures']['A'], s['structures']['B']
    assert a['soft_DSC'] == pytest.approx(8 / 9, rel=1e-12) and a['DSC_MAP'] == 1.0 and a['uncertain_vol'] == 1.0
    assert a['vol_mean'] == pytest.approx(1.25, rel=1e-12) and a['vol_std'] == pytest.approx(0.5, rel=1e-12)
    assert a['ECE'] == pytest.approx(0.125, rel=1e-12)
    assert b['soft_DSC'] == pytest.approx(0.5, rel=1e-12) and b['DSC_MAP'] == 1.0 and b['uncertain_vol'] == 2.0
    assert b['vol_mean'] == pytest.approx(1.0, rel=1e-12) and b['vol_std'] == pytest.approx(math.sqrt(2 / 3), rel=1e-12)
    assert b['ECE'] == 0.0 and s['ECE'] == pytest.approx(0.0625, rel=1e-12)
    assert s['entropy_mean'] == pytest.approx(2.5 * LN2 / 3, abs=1e-6) and s['entropy_max'] == pytest.approx(1.5 * LN2, abs=1e-6)
    check_against_restatement(lp, e, mp, s, label_posterior_np(records, fixed, [10, 16]))


def draw_case(C, steps, shape, K, seed):
    """K structures (some absent from every map), maps made of blobs with values in the dict, outside it and negative"""
    rng = np.random.default_rng(seed)
    labels = rng.choice(np.arange(-300, 300), size=K, replace=False).astype(int)
    absent = labels[: max(1, K // 4)] if K > 1 else []
    present = [x for x in labels if x not in absent] or list(labels)
    pool = np.array(present + [0, -7, 777, 1000])  # 0, negative and labels that are not in the dict are "other"
    pool = pool[~np.isin(pool, absent)]
    base = rng.choice(pool, size=shape)
    n = C * steps
    recs = np.repeat(base[None], n, axis=0)
    flip = rng.random((n, *shape)) < 0.3
    recs[flip] = rng.choice(pool, size=int(flip.sum()))
    fixed = np.where(rng.random(shape) < 0.7, base, rng.choice(pool, size=shape))
    structures = {f's{i}': int(x) for i, x in enumerate(labels)}
    return recs.astype(np.int16), fixed.astype(np.int16), structures


CASES = [  # C, steps, shape, K
    (1, 1, (1, 1, 3), 1),
    (2, 3, (1, 1, 3), 3),
    (3, 2, (5, 7, 9), 3),
    (8, 1, (5, 7, 9), 15),
    (2, 5, (17, 16, 33), 15),
    (1, 7, (17, 16, 33), 64),
    (3, 3, (64, 64, 64), 15),
    (8, 2, (64, 64, 64), 64),
]


@pytest.mark.parametrize('with_mask', [False, True])
@pytest.mark.parametrize('C,steps,shape,K', CASES)
def test_random_cases_match_the_restatement(C, steps, shape, K, with_mask):
    recs, fixed, structures = draw_case(C, steps, shape, K, seed=C * 1000 + steps * 10 + K)
    mask = (np.random.default_rng(K).random(shape) < 0.6) if with_mask else None
    spacing = (1.5, 0.75, 2.0)
    lp, e, mp, s = run_device(recs, C, fixed, structures, mask, spacing)
    ref = label_posterior_np(recs, fixed, list(structures.values()), mask)
    check_against_restatement(lp, e, mp, s, ref, spacing)
    assert lp.records == C * steps
    assert torch.equal(lp.probabilities(), lp.counts.float() / (C * steps))


def test_functional_form_and_an_empty_mask():
    recs, fixed, structures = draw_case(2, 3, (5, 7, 9), 3, seed=5)
    seg = torch.from_numpy(recs).to(DEV).reshape(3, 2, 1, 5, 7, 9).transpose(0, 1).contiguous()  # (C, N, 1, D, H, W)
    e, mp, s = calc_label_posterior(seg, torch.from_numpy(fixed), structures, (1, 1, 1))
    _, e2, mp2, s2 = run_device(recs, 2, fixed, structures)
    assert np.array_equal(e.cpu().numpy(), e2) and np.array_equal(mp.cpu().numpy(), mp2)
    assert np.array_equal(s['raw'], s2['raw'])
    _, _, _, s0 = run_device(recs, 2, fixed, structures, np.zeros((5, 7, 9), dtype=bool))
    assert s0['voxels'] == 0 and math.isnan(s0['entropy_mean']) and math.isnan(s0['entropy_max'])


def test_two_update_sequences_and_two_finalize_calls_are_bit_identical():
    recs, fixed, structures = draw_case(3, 4, (37, 41, 43), 15, seed=11)  # more than one block of partials
    mask = np.random.default_rng(2).random((37, 41, 43)) < 0.3
    a, ea, ma, sa = run_device(recs, 3, fixed, structures, mask)
    b, eb, mb, sb = run_device(recs, 3, fixed, structures, mask)
    assert torch.equal(a.counts, b.counts) and torch.equal(a.volume, b.volume)
    assert np.array_equal(ea, eb) and np.array_equal(ma, mb) and np.array_equal(sa['raw'], sb['raw'])
    m = torch.from_numpy(mask).to(DEV)
    f = torch.from_numpy(fixed).to(DEV)
    r1 = ops.label_posterior_finalize(a.counts, a.records, a.labels, f, m)
    r2 = ops.label_posterior_finalize(a.counts, a.records, a.labels, f, m)
    for u, v in zip(r1, r2):
        assert torch.equal(u, v)
    assert r1[3].dtype == torch.float64 and int(r1[3][0]) == int(mask.sum())


def test_abi_and_python_refusals():
    lib = L.load()
    Cn, K, D, H, W = 2, 3, 4, 5, 6
    labels = [10, 16, 20]
    lab = (C.c_int32 * K)(*labels)
    seg = torch.zeros(Cn, 1, D, H, W, device=DEV, dtype=torch.int16)
    counts = torch.zeros(K, D, H, W, device=DEV, dtype=torch.int32)
    volume = torch.zeros(K, 2, device=DEV, dtype=torch.float64)
    fixed = torch.zeros(D, H, W, device=DEV, dtype=torch.int16)
    ent = torch.empty(D, H, W, device=DEV)
    mp = torch.empty(D, H, W, device=DEV, dtype=torch.int16)
    summ = torch.empty(K, 6 + 3 * BINS, device=DEV, dtype=torch.int64)
    ms = torch.empty(4, device=DEV, dtype=torch.float64)
    nb = C.c_size_t()
    L.check(lib.irs_label_posterior_workspace(Cn, K, D, H, W, C.byref(nb)))
    ws = torch.empty(nb.value, device=DEV, dtype=torch.uint8)
    q = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    st = L.stream_ptr()

    def upd(seg_=seg, C_=Cn, labels_=lab, K_=K, counts_=counts, volume_=volume, before=0, ws_=ws, ws_bytes=nb.value):
        return lib.irs_label_posterior_update(q(seg_), C_, D, H, W, labels_, K_, q(counts_), q(volume_), before, q(ws_),
                                              ws_bytes, st)

    def fin(counts_=counts, K_=K, n=2, labels_=lab, fixed_=fixed, ent_=ent, mp_=mp, summ_=summ, ms_=ms, ws_=ws,
            ws_bytes=nb.value):
        return lib.irs_label_posterior_finalize(q(counts_), K_, D, H, W, n, labels_, q(fixed_), None, q(ent_), q(mp_),
                                                q(summ_), q(ms_), q(ws_), ws_bytes, st)

    L.check(upd())
    L.check(fin())
    torch.cuda.synchronize()
    dup = (C.c_int32 * K)(10, 16, 10)
    for kw in (dict(seg_=None), dict(counts_=None), dict(volume_=None), dict(ws_=None), dict(C_=0), dict(C_=9),
               dict(K_=0), dict(K_=65), dict(labels_=dup), dict(before=-1), dict(before=2 ** 31 - 2),
               dict(ws_bytes=4)):  # the update needs 4 * C * K bytes per block of partials
        with pytest.raises(L.IrsError):
            L.check(upd(**kw))
    for kw in (dict(counts_=None), dict(fixed_=None), dict(ent_=None), dict(mp_=None), dict(summ_=None), dict(ms_=None),
               dict(ws_=None), dict(K_=0), dict(K_=65), dict(labels_=dup), dict(n=0), dict(n=-1), dict(ws_bytes=8)):
        with pytest.raises(L.IrsError):
            L.check(fin(**kw))
    # nothing was counted by a refused call
    torch.cuda.synchronize()
    assert int(counts.sum()) == 0
    # the Python surface checks shapes and dtypes before it calls
    with pytest.raises(L.IrsError):
        ops.label_posterior_update(seg.int(), labels, counts, volume, 0)
    with pytest.raises(L.IrsError):
        ops.label_posterior_update(seg[:, :, :2], labels, counts, volume, 0)
    with pytest.raises(L.IrsError):
        ops.label_posterior_update(seg, labels, counts.long(), volume, 0)
    with pytest.raises(L.IrsError):
        ops.label_posterior_update(seg, labels, counts, volume.float(), 0)
    with pytest.raises(L.IrsError):
        ops.label_posterior_update(seg, labels[:2], counts, volume, 0)
    with pytest.raises(L.IrsError):
        ops.label_posterior_update(seg.cpu(), labels, counts, volume, 0)
    with pytest.raises(L.IrsError):
        ops.label_posterior_finalize(counts, 2, labels[:2], fixed)
    with pytest.raises(L.IrsError):
        ops.label_posterior_finalize(counts, 2, labels, fixed[:, :, :3])
    with pytest.raises(L.IrsError):
        ops.label_posterior_finalize(counts, 2, labels, fixed, mask=torch.ones(D, H, W + 1, device=DEV, dtype=torch.bool))
    with pytest.raises(L.IrsError):
        ops.label_posterior_finalize(counts, 0, labels, fixed)


def test_a_wrong_record_count_is_caught_by_the_inconsistency_count():
    records = np.array([[10, 10, 0], [10, 16, 0], [10, 16, 16], [10, 0, 16]]).reshape(4, 1, 1, 3)
    lp, _, _, _ = run_device(records, 2, np.array([10, 16, 0]).reshape(1, 1, 3), {'A': 10, 'B': 16})
    _, _, _, ms = ops.label_posterior_finalize(lp.counts, 3, lp.labels, torch.zeros(1, 1, 3, dtype=torch.int16, device=DEV))
    assert ms.cpu().tolist()[3] == 1.0  # voxel 0 holds A four times
    lp.records = 3
    with pytest.raises(L.IrsError, match='more than the 3 records'):
        lp.finalize(torch.zeros(1, 1, 3, dtype=torch.int16))


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


def nifti_datatype(path):
    import gzip
    import struct
    with gzip.open(str(path), 'rb') as f:
        return struct.unpack('<h', f.read(72)[70:72])[0]


def test_trainer_maps_match_the_recorded_warps(tmp_path, monkeypatch):
    from ir_sgmcmc_amd.utils.imageio import read_nifti
    N = 24
    kept = []
    record = LabelPosterior.record

    def spy(self, seg_warped):
        kept.append(seg_warped.clone())
        return record(self, seg_warped)

    monkeypatch.setattr(LabelPosterior, 'record', spy)
    kw = dict(no_iters_burn_in=3, no_samples_MCMC=9, log_period_MCMC=4, convergence_diagnostics={'period': 1})
    torch.manual_seed(0)
    t = make_trainer(tmp_path / 'on', (N, N, N), label_posterior={'period': 2, 'prob_maps': True}, **kw)
    t.run()
    C = t.no_chains
    assert len(kept) == len(recorded_steps(3, 9, 2)) == 9 // 2 and t._label_posterior.records == C * (9 // 2)
    records = torch.cat(kept).reshape(-1, N, N, N).cpu().numpy()  # steps in order, chains in order within a step
    fixed_data = next(iter(t.data_loader))[0]
    seg_fixed = fixed_data['seg'].reshape(N, N, N).numpy()
    mask = fixed_data['mask'].reshape(N, N, N).numpy() != 0
    structures = t.structures_dict
    ref = label_posterior_np(records, seg_fixed, list(structures.values()), mask)
    spacing = t.data_loader.im_spacing if getattr(t.data_loader, 'im_spacing', None) is not None else torch.ones(3)
    sp = [float(x) for x in spacing]
    lp = t._label_posterior
    check_against_restatement(lp, t.label_entropy.cpu().numpy(), t.label_map.cpu().numpy(), t.label_summary, ref, sp)
    # files
    folder = t.config.save_dirs['samples']
    ent, _ = read_nifti(str(folder / 'MCMC_seg_entropy.nii.gz'))
    assert np.array_equal(ent, t.label_entropy.cpu().numpy())
    masked, _ = read_nifti(str(folder / 'MCMC_seg_entropy_masked.nii.gz'))
    assert np.array_equal(masked[mask], ent[mask]) and not masked[~mask].any()
    mp, _ = read_nifti(str(folder / 'MCMC_seg_MAP.nii.gz'), dtype=np.int16)
    assert nifti_datatype(folder / 'MCMC_seg_MAP.nii.gz') == 4 and np.array_equal(mp, t.label_map.cpu().numpy())  # int16
    prob = lp.probabilities().cpu().numpy()
    for j, name in enumerate(structures):
        p, _ = read_nifti(str(folder / f'MCMC_seg_prob_{name}.nii.gz'))
        assert nifti_datatype(folder / f'MCMC_seg_prob_{name}.nii.gz') == 16 and np.array_equal(p, prob[j])  # float32
    # metrics
    res = t.metrics.result()
    for name, st in t.label_summary['structures'].items():
        for k, v in st.items():
            got = res[f'MCMC/seg/{name}/{k}']
            assert (math.isnan(got) and math.isnan(v)) or got == v
    for k in ('entropy_mean', 'entropy_max', 'ECE'):
        assert res[f'MCMC/seg/{k}'] == t.label_summary[k]
    # the same run with the option off: bit-identical displacement moments and R-hat, and no label anything
    monkeypatch.setattr(LabelPosterior, 'record', record)
    torch.manual_seed(0)
    off = make_trainer(tmp_path / 'off', (N, N, N), **kw)
    off.run()
    assert torch.equal(off.displacement_mean, t.displacement_mean) and torch.equal(off.displacement_std, t.displacement_std)
    assert torch.equal(off.rhat, t.rhat)
    assert off.label_entropy is None and off.label_map is None and off.label_summary is None
    assert not [k for k in off.metrics.result() if k.startswith('MCMC/seg/')]
    assert not list(off.config.save_dirs['samples'].glob('*_seg_*'))


def test_trainer_label_posterior_survives_checkpoint_resume_bit_for_bit(tmp_path):
    kw = dict(no_iters_burn_in=2, no_samples_MCMC=8, log_period_MCMC=4, checkpoint_period=6, label_posterior={'period': 2},
              save_outputs=False)
    a = make_trainer(tmp_path / 'a', (16, 16, 16), **kw)
    a.run()
    ck = a.config.save_dirs['checkpoints'] / 'checkpoint_0000006.pt'
    sd = torch.load(ck, map_location='cpu', weights_only=True)
    assert sd['label_posterior']['records'] == 2 * a.no_chains and sd['label_posterior']['labels'] == list(a.structures_dict.values())
    b = make_trainer(tmp_path / 'b', (16, 16, 16), resume=str(ck), **kw)
    b.run()
    assert torch.equal(a.label_entropy, b.label_entropy) and torch.equal(a.label_map, b.label_map)
    assert np.array_equal(a.label_summary['raw'], b.label_summary['raw'])
    assert torch.equal(a._label_posterior.volume, b._label_posterior.volume)
    # a checkpoint without the key, once a recorded step has passed, is refused; the option off keeps the key set
    del sd['label_posterior']
    ck2 = tmp_path / 'no_labels.pt'
    torch.save(sd, ck2)
    c = make_trainer(tmp_path / 'c', (16, 16, 16), resume=str(ck2), **kw)
    with pytest.raises(ValueError, match='label_posterior'):
        c.run()
    off_kw = {k: v for k, v in kw.items() if k != 'label_posterior'}
    off = make_trainer(tmp_path / 'off', (16, 16, 16), **off_kw)
    off.run()
    sd_off = torch.load(off.config.save_dirs['checkpoints'] / 'checkpoint_0000006.pt', map_location='cpu', weights_only=True)
    assert set(sd_off) == set(sd)
