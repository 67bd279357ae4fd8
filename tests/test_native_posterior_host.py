"""Native-grid posteriors without a GPU: the option parser, the numpy restatement of tests/_native_posterior.py on the cases
whose answer is exact (a zero field, integer translations on the dyadic geometry), and the recorder's state_dict."""
import numpy as np
import pytest
import torch

from ir_sgmcmc_amd.diagnostics import (LABEL_STRUCTURE_METRICS, NativePosterior, native_posterior_metric_names,
                                       native_posterior_options)
from ir_sgmcmc_amd.native import NativeGrid
from tests import _native_posterior as NP
from tests import _native_resolution as R

BASE = {'log_period_MCMC': 4, 'no_samples_MCMC': 8, 'no_chains': 2, 'native_resolution': True}
LABELS = [1, 3, 7]          # 7 is absent from the maps of R.random_volumes (labels 0 .. 5); 2, 4, 5 count as "other"
DYADIC = NativeGrid.from_shape((9, 17, 17), (9, 9, 9))   # p = (4, 0, 0), P = 17^3, grid step 0.5
# (constant displacement per channel, the integer source offset per axis it gives): tests/test_gpu_native_resolution.py
SHIFTS = [((2 * 2 / 16, 0.0, -2 * 1 / 16), (-1, 0, 2)), ((0.0, 0.0, 2 * 6 / 16), (6, 0, 0)), ((2 * 20 / 16, 0.0, 0.0), (0, 0, 20))]


# ---------------------------------------------------------------- options
@pytest.mark.parametrize('opt', [None, False])
def test_option_off(opt):
    assert native_posterior_options({**BASE, 'native_posterior': opt}) is None
    assert native_posterior_options(BASE) is None
    assert native_posterior_options({'log_period_MCMC': 4, 'no_samples_MCMC': 8}) is None   # off needs nothing else


def test_option_forms():
    assert native_posterior_options({**BASE, 'native_posterior': True}) == {
        'period': 4, 'labels': True, 'image': True, 'prob_maps': False, 'std_floor': None}
    got = native_posterior_options({**BASE, 'native_posterior': {'period': 2, 'image': False, 'prob_maps': True, 'std_floor': 0}})
    assert got == {'period': 2, 'labels': True, 'image': False, 'prob_maps': True, 'std_floor': 0.0}
    assert native_posterior_options({**BASE, 'native_resolution': {'period': 3}, 'native_posterior': {'labels': False}})['image']


@pytest.mark.parametrize('opt, message', [
    ({'perid': 2}, 'unknown keys'),
    ('yes', 'must be true, false or'),
    ({'period': 0}, 'period must be >= 1'),
    ({'period': 2.0}, 'period must be an integer'),
    ({'period': True}, 'period must be an integer'),
    ({'period': 9}, 'records no step'),
    ({'labels': False, 'image': False}, 'both false'),
    ({'labels': 1}, 'labels must be true or false'),
    ({'image': 'no'}, 'image must be true or false'),
    ({'prob_maps': None}, 'prob_maps must be true or false'),
    ({'std_floor': -0.5}, 'std_floor must be a finite number >= 0 or null'),
    ({'std_floor': float('inf')}, 'std_floor must be a finite number >= 0 or null'),
    ({'std_floor': '1'}, 'std_floor must be a finite number >= 0 or null'),
])
def test_option_refusals(opt, message):
    with pytest.raises(ValueError, match=message):
        native_posterior_options({**BASE, 'native_posterior': opt})


@pytest.mark.parametrize('native', [None, False, 'absent'])
def test_option_needs_native_resolution(native):
    cfg = {**BASE, 'native_posterior': True, 'native_resolution': native}
    if native == 'absent':
        del cfg['native_resolution']
    with pytest.raises(ValueError, match='needs trainer.native_resolution'):
        native_posterior_options(cfg)


def test_option_labels_need_segmentations():
    class NoSegs:
        has_segs = False
    with pytest.raises(ValueError, match='"labels" needs the fixed and the moving segmentation'):
        native_posterior_options({**BASE, 'native_posterior': True}, NoSegs())
    assert native_posterior_options({**BASE, 'native_posterior': {'labels': False}}, NoSegs())['labels'] is False


def test_metric_names():
    names = native_posterior_metric_names({'labels': True, 'image': True}, {'a': 1, 'b': 2})
    assert len(names) == len(set(names)) == 2 * len(LABEL_STRUCTURE_METRICS) + 3 + 6
    assert 'MCMC/native/seg/vol_mean/b' in names and 'MCMC/native/seg/ECE' in names and 'MCMC/native/image/moving/z_gt3' in names
    assert all('/seg/' not in k for k in native_posterior_metric_names({'labels': False, 'image': True}, {'a': 1}))


# ---------------------------------------------------------------- the restatement on the exact cases
@pytest.mark.parametrize('shape, dims', [((10, 13, 16), (8, 8, 8)), ((6, 7, 5), (16, 16, 16))])
@pytest.mark.parametrize('C, Cim', [(1, 1), (3, 1), (2, 2)])
def test_zero_field(shape, dims, C, Cim):
    grid = NativeGrid.from_shape(shape, dims)
    im, seg, _ = (t.numpy()[:, 0] for t in R.random_volumes(shape, 6, Cim))
    got = NP.native_posterior_np([np.zeros((C, 3, *dims), np.float32)], grid, seg, LABELS, im, float(im.min()))
    want = sum((seg[c if Cim > 1 else 0][None] == np.asarray(LABELS).reshape(-1, 1, 1, 1)).astype(np.int64) for c in range(C))
    assert np.array_equal(got['counts'], want) and got['records'] == C
    if Cim == 1:   # C records of one map: the mean is the voxel count, no spread; the image comes back bit for bit
        assert np.array_equal(got['vol_mean'], want.reshape(len(LABELS), -1).sum(1) / C) and not got['vol_m2'].any()
        assert np.array_equal(got['mean'].view(np.int32), im[0].view(np.int32)) and not got['m2'].any()
        assert np.array_equal(got['low'], im[0]) and np.array_equal(got['high'], im[0])
    assert got['counts'][2].sum() == 0 and got['counts'].sum() < C * seg[0].size   # the absent label; "other" exists


@pytest.mark.parametrize('per_channel, shift', SHIFTS)
def test_integer_translations(per_channel, shift):
    im, seg, _ = R.random_volumes(DYADIC.shape, 5)
    fill = float(im.min())
    u = R.constant_field(2, DYADIC.dims, per_channel).numpy()
    got = NP.native_posterior_np([u], DYADIC, seg.numpy()[:, 0], LABELS, im.numpy()[:, 0], fill)
    seg_want = R.shifted(seg, DYADIC, shift, 0)[0, 0].numpy()
    im_want = R.shifted(im, DYADIC, shift, fill)[0, 0].numpy()
    assert np.array_equal(got['counts'], 2 * (seg_want[None] == np.asarray(LABELS).reshape(-1, 1, 1, 1)))
    assert np.array_equal(got['mean'], im_want) and not got['m2'].any()
    assert np.array_equal(got['low'], im_want) and np.array_equal(got['high'], im_want)
    assert np.array_equal(got['vol_mean'], (seg_want[None] == np.asarray(LABELS).reshape(-1, 1, 1, 1)).reshape(3, -1).sum(1))
    if shift == (6, 0, 0):   # beyond the pad of the first axis: the fill for the image, "other" for the labels
        assert (got['mean'][3:] == fill).all() and not got['counts'][:, 3:].any()


# ---------------------------------------------------------------- the recorder's state
def make(grid=DYADIC, structures=None, seg=True, im=True):
    shape = grid.shape
    return NativePosterior(grid, 'cpu', structures or {'a': 1, 'b': 3}, torch.zeros(1, 1, *shape, dtype=torch.int16) if seg else None,
                           torch.zeros(1, 1, *shape) if im else None, 0.0)


def test_state_dict_round_trip():
    a = make()
    a.state['counts'].random_(0, 5)
    a.state['volume'].normal_()
    for key in ('mean', 'm2', 'low', 'high'):
        a.state[key].normal_()
    a.records = 6
    assert a.state_bytes() == (4 * 2 + 16) * 9 * 17 * 17 + 32
    sd = a.state_dict()
    assert all(torch.is_tensor(v) or isinstance(v, (int, bool, list)) for v in sd.values())   # a checkpoint is data
    b = make()
    b.load_state_dict(sd)
    assert b.records == 6 and all(torch.equal(a.state[k], b.state[k]) for k in a.state)
    assert torch.equal(b.probabilities(), a.state['counts'].float() / 6)


def test_state_dict_refusals():
    sd = make().state_dict()
    with pytest.raises(ValueError, match='labels'):
        make(structures={'a': 1, 'b': 4}).load_state_dict(sd)
    with pytest.raises(ValueError, match='labels'):
        make(structures={'a': 1}).load_state_dict(sd)
    with pytest.raises(ValueError, match='geometry'):
        make(NativeGrid.from_shape((9, 17, 17), (8, 9, 9))).load_state_dict(sd)      # other dims
    with pytest.raises(ValueError, match='geometry'):
        make(NativeGrid.from_shape((9, 17, 16), (9, 9, 9))).load_state_dict(sd)      # other shape
    with pytest.raises(ValueError, match='image part'):
        make(im=False).load_state_dict(sd)
    with pytest.raises(ValueError, match='labels'):
        make(seg=False).load_state_dict(sd)
    bad = dict(sd, mean=sd['mean'][1:])
    with pytest.raises(ValueError, match="state 'mean' of shape"):
        make().load_state_dict(bad)


def test_recorder_refusals():
    with pytest.raises(ValueError, match='neither'):
        make(seg=False, im=False)
    with pytest.raises(ValueError, match='not distinct'):
        make(structures={'a': 1, 'b': 1})
    with pytest.raises(ValueError, match='finite fill'):
        NativePosterior(DYADIC, 'cpu', None, None, torch.zeros(1, 1, *DYADIC.shape), None)
    with pytest.raises(RuntimeError, match='nothing recorded'):
        make().finalize()
