"""Posterior label maps, host side: the known answer of the definitions against the numpy restatement, the config option and
its refusals, the metric names, and the parts of the surface that need no device."""
import copy
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

from ir_sgmcmc_amd import _lib as L
from ir_sgmcmc_amd.diagnostics import LabelPosterior, label_posterior_options, label_summary
from tests._label_posterior import BINS, derived_np, label_posterior_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = {'no_samples_MCMC': 80, 'log_period_MCMC': 10, 'no_chains': 2}
LN2 = math.log(2.0)

# the known answer: (D,H,W) = (1,1,3), labels {A: 10, B: 16}, two chains, two steps
KA_LABELS = {'A': 10, 'B': 16}
KA_RECORDS = np.array([[10, 10, 0], [10, 16, 0], [10, 16, 16], [10, 0, 16]]).reshape(4, 1, 1, 3)
KA_FIXED = np.array([10, 16, 0]).reshape(1, 1, 3)


def _config(tmp_path, **trainer_over):
    from ir_sgmcmc_amd.parse_config import ConfigParser
    cfg = json.load(open(os.path.join(ROOT, 'configs', 'synthetic_gmm_lognormal.json')))
    cfg['trainer']['save_dir'] = str(tmp_path)
    cfg['trainer'].update(trainer_over)
    return ConfigParser.from_dict(copy.deepcopy(cfg), timestamp='t')


# ---------------------------------------------------------------- the known answer
def test_known_answer_of_the_restatement():
    ref = label_posterior_np(KA_RECORDS, KA_FIXED, list(KA_LABELS.values()))
    assert ref['counts'].reshape(2, 3).tolist() == [[4, 1, 0], [0, 2, 2]]
    assert np.allclose(ref['entropy'].reshape(-1), [0.0, 1.5 * LN2, LN2], atol=1e-15, rtol=0)
    assert ref['map'].reshape(-1).tolist() == [10, 16, 0]  # voxel 2: other and B tie at 2, other wins
    per, ece, e_mean, e_max = derived_np(ref)
    a, b = per
    assert a['soft_DSC'] == pytest.approx(8 / 9, rel=1e-15) and a['DSC_MAP'] == 1.0 and a['uncertain_vol'] == 1
    assert ref['vol'][:, 0].tolist() == [2, 1, 1, 1] and a['vol_mean'] == 1.25 and a['vol_std'] == pytest.approx(0.5, rel=1e-15)
    assert a['ECE'] == pytest.approx(0.125, rel=1e-15)
    assert b['soft_DSC'] == 0.5 and b['DSC_MAP'] == 1.0 and b['uncertain_vol'] == 2
    assert ref['vol'][:, 1].tolist() == [0, 1, 2, 1] and b['vol_mean'] == 1.0
    assert b['vol_std'] == pytest.approx(math.sqrt(2 / 3), rel=1e-15) and b['ECE'] == 0.0
    # A's pairs fall in bins 9 (c = 4) and 2 (c = 1); B's both in bin 5 (c = 2)
    bins = ref['summary'][:, 6:].reshape(2, BINS, 3)
    assert bins[0, :, 0].nonzero()[0].tolist() == [2, 9] and bins[1, :, 0].nonzero()[0].tolist() == [5]
    assert bins[1, 5].tolist() == [2, 4, 1]
    assert ece == pytest.approx(0.0625, rel=1e-15)
    assert e_mean == pytest.approx(2.5 * LN2 / 3, abs=1e-7) and e_max == pytest.approx(1.5 * LN2, abs=1e-7)
    # the Welford fold gives the same moments as the two-pass formulas
    assert ref['vol_mean'].tolist() == [1.25, 1.0]
    assert ref['vol_m2'] == pytest.approx([0.75, 2.0], rel=1e-15)


def test_label_summary_turns_the_sums_into_the_known_answer():
    ref = label_posterior_np(KA_RECORDS, KA_FIXED, list(KA_LABELS.values()))
    volume = np.stack([ref['vol_mean'], ref['vol_m2']], axis=1)
    ms = [3.0, ref['entropy_sum'], ref['entropy_max'], 0.0]
    s = label_summary(ref['summary'], volume, 4, ms, list(KA_LABELS), (1.0, 2.0, 0.5))
    a, b = s['structures']['A'], s['structures']['B']
    assert a['soft_DSC'] == pytest.approx(8 / 9) and a['DSC_MAP'] == 1.0 and a['ECE'] == pytest.approx(0.125)
    assert a['vol_mean'] == 1.25 and a['vol_std'] == pytest.approx(0.5) and a['uncertain_vol'] == 1.0  # v = 1 mm^3
    assert b['vol_std'] == pytest.approx(math.sqrt(2 / 3)) and b['uncertain_vol'] == 2.0 and b['ECE'] == 0.0
    assert s['ECE'] == pytest.approx(0.0625) and s['voxels'] == 3 and s['records'] == 4
    assert s['entropy_mean'] == pytest.approx(2.5 * LN2 / 3, abs=1e-7)
    # 0 / 0 is NaN, as calc_DSC_GPU has it; an empty mask gives NaN mean and max
    empty = label_summary(np.zeros((1, 6 + 3 * BINS), dtype=np.int64), np.zeros((1, 2)), 3, [0.0, 0.0, 0.0, 0.0], ['X'],
                          (1, 1, 1))
    x = empty['structures']['X']
    assert math.isnan(x['soft_DSC']) and math.isnan(x['DSC_MAP']) and math.isnan(x['ECE']) and x['vol_std'] == 0.0
    assert math.isnan(empty['entropy_mean']) and math.isnan(empty['entropy_max']) and math.isnan(empty['ECE'])


def test_restatement_tie_rules_and_other_class():
    # negative values and labels outside the dict are "other"; ties between structures go to the first one
    recs = np.array([[-3, 5, 7], [5, 7, 7], [99, 5, 5], [-3, 7, 5]]).reshape(4, 1, 1, 3)
    ref = label_posterior_np(recs, np.zeros((1, 1, 3), dtype=int), [7, 5])
    assert ref['counts'].reshape(2, 3).tolist() == [[0, 2, 2], [1, 2, 2]]
    assert ref['map'].reshape(-1).tolist() == [0, 7, 7]
    assert ref['entropy'][0, 0, 0] == pytest.approx(-(0.75 * math.log(0.75) + 0.25 * math.log(0.25)), rel=1e-14)


# ---------------------------------------------------------------- the config option
def test_option_values():
    assert label_posterior_options(BASE) is None
    for off in (False, None):
        assert label_posterior_options({**BASE, 'label_posterior': off}) is None
    assert label_posterior_options({**BASE, 'label_posterior': True}) == {'period': 10, 'prob_maps': False}
    assert label_posterior_options({**BASE, 'label_posterior': {}}) == {'period': 10, 'prob_maps': False}
    assert label_posterior_options({**BASE, 'label_posterior': {'period': 3}}) == {'period': 3, 'prob_maps': False}
    assert label_posterior_options({**BASE, 'label_posterior': {'prob_maps': True}}) == {'period': 10, 'prob_maps': True}
    assert label_posterior_options({**BASE, 'label_posterior': {'period': 80, 'prob_maps': False}})['period'] == 80


@pytest.mark.parametrize('opt', [{'period': 0}, {'period': -2}, {'period': 2.5}, {'period': 2.0}, {'period': '2'},
                                 {'period': True}, {'period': None}, {'prob_maps': 1}, {'prob_maps': 'yes'},
                                 {'prob_maps': None}, {'periods': 2}, {'period': 2, 'maps': True}, 'yes', 1, [2]])
def test_option_refusals(opt):
    with pytest.raises(ValueError, match='label_posterior'):
        label_posterior_options({**BASE, 'label_posterior': opt})


def test_a_config_that_records_nothing_or_too_much_is_refused():
    with pytest.raises(ValueError, match=r'label_posterior: no_samples_MCMC = 80 with period 81 records no step'):
        label_posterior_options({**BASE, 'label_posterior': {'period': 81}})
    big = {'no_samples_MCMC': 2 ** 31, 'log_period_MCMC': 1, 'no_chains': 2}
    with pytest.raises(ValueError, match='label_posterior.*at most 2147483647'):
        label_posterior_options({**big, 'label_posterior': True})
    with pytest.raises(ValueError, match='label_posterior.*2147483648 records'):
        label_posterior_options({**big, 'label_posterior': {'period': 2}})  # 2^30 steps x 2 chains
    assert label_posterior_options({**big, 'no_chains': 1, 'label_posterior': {'period': 2}})['period'] == 2
    edge = {'no_samples_MCMC': 2 ** 31 - 1, 'log_period_MCMC': 1, 'no_chains': 1}
    assert label_posterior_options({**edge, 'label_posterior': True})['period'] == 1


def test_trainer_refuses_the_config_when_it_is_built(tmp_path):
    from ir_sgmcmc_amd.trainer import Trainer
    config = _config(tmp_path, no_samples_MCMC=4, log_period_MCMC=2, label_posterior={'period': 5})
    dl = config.init_data_loader()
    losses = config.init_losses()
    tm, rm = config.init_transformation_and_registration_modules()
    with pytest.raises(ValueError, match='label_posterior'):
        config.init_metrics()
    with pytest.raises(ValueError, match='label_posterior'):
        Trainer(config, dl, losses, tm, rm, [], device='cpu')


def test_init_metrics_names_the_label_posterior_after_ess_only_when_on(tmp_path):
    off = _config(tmp_path / 'off').init_metrics()
    assert not [k for k in off if k.startswith('MCMC/seg/')]
    on = _config(tmp_path / 'on', label_posterior=True).init_metrics()
    structures = _config(tmp_path / 'names').structures_dict
    seg = [f'MCMC/seg/{s}/{k}' for s in structures for k in ('soft_DSC', 'DSC_MAP', 'vol_mean', 'vol_std', 'uncertain_vol', 'ECE')]
    seg += ['MCMC/seg/entropy_mean', 'MCMC/seg/entropy_max', 'MCMC/seg/ECE']
    assert on == off + seg
    ess = {'period': 5, 'ess': True}
    both = _config(tmp_path / 'both', convergence_diagnostics=ess, label_posterior={'period': 4}).init_metrics()
    assert both == _config(tmp_path / 'ess', convergence_diagnostics=ess).init_metrics() + seg


# ---------------------------------------------------------------- device-free parts of the surface
def test_label_posterior_state_and_refusals():
    lp = LabelPosterior(KA_LABELS, (1, 1, 3), 'cpu')
    assert tuple(lp.counts.shape) == (2, 1, 1, 3) and lp.counts.dtype == torch.int32
    assert tuple(lp.volume.shape) == (2, 2) and lp.volume.dtype == torch.float64
    with pytest.raises(L.IrsError):
        lp.record(torch.zeros(2, 1, 1, 1, 3, dtype=torch.int16))  # CPU tensors never reach the library
    assert lp.records == 0
    sd = lp.state_dict()
    assert set(sd) == {'counts', 'volume', 'records', 'labels'} and sd['labels'] == [10, 16]
    sd['records'] = 6
    sd['counts'] = torch.full_like(sd['counts'], 3)
    other = LabelPosterior(KA_LABELS, (1, 1, 3), 'cpu')
    other.load_state_dict(sd)
    assert other.records == 6 and torch.equal(other.counts, sd['counts'])
    with pytest.raises(ValueError, match='labels'):
        LabelPosterior({'A': 10, 'B': 17}, (1, 1, 3), 'cpu').load_state_dict(sd)
    with pytest.raises(ValueError, match='shape'):
        LabelPosterior(KA_LABELS, (1, 1, 4), 'cpu').load_state_dict(sd)
    with pytest.raises(ValueError):
        LabelPosterior({}, (1, 1, 3), 'cpu')
    with pytest.raises(ValueError):
        LabelPosterior({'A': 10, 'B': 10}, (1, 1, 3), 'cpu')
    with pytest.raises(ValueError):
        LabelPosterior({f's{i}': i for i in range(65)}, (1, 1, 3), 'cpu')


def test_workspace_size_and_refusals_without_a_device():
    lib = L.load()
    n = C.c_size_t()
    assert lib.irs_label_posterior_workspace(2, 15, 1, 1, 3, C.byref(n)) == 0 and n.value > 0
    assert lib.irs_label_posterior_workspace(2, 15, 256, 256, 256, C.byref(n)) == 0
    assert n.value == 1024 * (15 * (6 + 3 * BINS) * 8 + 4 * 8)  # the finalize's partials of a capped grid
    for bad in ((0, 15, 4, 4, 4), (9, 15, 4, 4, 4), (2, 0, 4, 4, 4), (2, 65, 4, 4, 4), (2, 15, 0, 4, 4), (2, 15, 4, -1, 4)):
        assert lib.irs_label_posterior_workspace(*bad, C.byref(n)) != 0
    assert lib.irs_label_posterior_workspace(2, 15, 4, 4, 4, None) != 0
    p = C.c_void_p(16)  # never dereferenced: every call below is refused before a launch
    lab = (C.c_int32 * 3)(10, 16, 10)
    ok = (C.c_int32 * 3)(10, 16, 20)
    big = 1 << 30

    def upd(seg=p, Cn=2, D=4, H=4, W=4, labels=ok, K=3, counts=p, volume=p, before=0, ws=p, ws_bytes=big):
        return lib.irs_label_posterior_update(seg, Cn, D, H, W, labels, K, counts, volume, before, ws, ws_bytes, None)

    def fin(counts=p, K=3, D=4, H=4, W=4, n=4, labels=ok, seg=p, mask=None, ent=p, mp=p, summ=p, ms=p, ws=p, ws_bytes=big):
        return lib.irs_label_posterior_finalize(counts, K, D, H, W, n, labels, seg, mask, ent, mp, summ, ms, ws, ws_bytes, None)

    for kw, msg in ((dict(labels=lab), 'twice'), (dict(Cn=0), 'chains'), (dict(Cn=9), 'chains'), (dict(K=0), 'labels'),
                    (dict(K=65), 'labels'), (dict(before=-1), 'records_before'), (dict(before=2 ** 31 - 2), 'overflow'),
                    (dict(ws_bytes=8), 'workspace'), (dict(seg=None), 'bad'), (dict(counts=None), 'bad'),
                    (dict(volume=None), 'bad'), (dict(ws=None), 'bad'), (dict(D=0), 'bad'),
                    (dict(labels=(C.c_int32 * 3)(10, 16, 40000)), 'int16')):
        assert upd(**kw) != 0, kw
        assert msg in lib.irs_last_error().decode(), (kw, lib.irs_last_error())
    for kw, msg in ((dict(labels=lab), 'twice'), (dict(n=0), 'n = 0'), (dict(n=-4), 'n = -4'), (dict(K=0), 'labels'),
                    (dict(K=65), 'labels'), (dict(ws_bytes=8), 'workspace'), (dict(counts=None), 'bad'),
                    (dict(seg=None), 'bad'), (dict(ent=None), 'bad'), (dict(mp=None), 'bad'), (dict(summ=None), 'bad'),
                    (dict(ms=None), 'bad'), (dict(ws=None), 'bad'), (dict(W=0), 'bad')):
        assert fin(**kw) != 0, kw
        assert msg in lib.irs_last_error().decode(), (kw, lib.irs_last_error())
