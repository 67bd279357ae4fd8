"""Native-grid posteriors on the device.  The yardstick is the composition of operators that exist without the fused kernel:
ops.native_warp(seg, im), ops.label_posterior_update on the native extents and tests/_image_posterior.welford32 / min / max on the
host.  Counts and volumes must be equal, the image state equal bit for bit.  Then the exact cases of
tests/test_native_posterior_host.py, the instantiations, determinism, the first record, every refusal, the mm^3 of the
finalize and the trainer option."""
import copy
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from ir_sgmcmc_amd import _lib as L
from ir_sgmcmc_amd import native_posterior as P
from ir_sgmcmc_amd import ops as G
from ir_sgmcmc_amd.diagnostics import NativePosterior, label_summary, native_posterior_metric_names
from ir_sgmcmc_amd.native import NativeGrid
from ir_sgmcmc_amd.parse_config import ConfigParser
from ir_sgmcmc_amd.trainer import Trainer
from ir_sgmcmc_amd.utils import calc_native_posterior
from ir_sgmcmc_amd.utils.imageio import read_nifti
from tests import _native_posterior as NP
from tests import _native_resolution as R
from tests._image_posterior import welford32
from tests.test_native_posterior_host import DYADIC, LABELS, SHIFTS

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMAGE = P.IMAGE_KEYS


def dev(t):
    return t.to(DEV).contiguous()


def bits(t):
    return t.contiguous().view(torch.int32)


def volumes(shape, seed, Cim=1):
    """image and segmentation of R.random_volumes (labels 0 .. 5) with label 5 turned into -2: with LABELS = [1, 3, 7] the map holds
    values outside the set (0, 2, 4), a negative one, and 7 is absent"""
    im, seg, _ = R.random_volumes(shape, seed, Cim)
    seg[seg == 5] = -2
    return im, seg


def fused(steps, grid, seg=None, im=None, fill=None, labels=LABELS, state=None, records_before=0):
    """the steps folded by the operator under test -> (state, records)"""
    if state is None:
        state = P.native_posterior_state(grid, labels if seg is not None else None, im is not None, DEV)
    n = records_before
    for u in steps:
        P.native_posterior_update(dev(u), grid, state, n, seg=None if seg is None else dev(seg), im=None if im is None else dev(im),
                                  fill=fill)
        n += u.shape[0]
    return state, n


def composition(steps, grid, seg, im, fill, labels=LABELS):
    """the same state from ops.native_warp, ops.label_posterior_update and the host Welford fold"""
    counts = torch.zeros((len(labels), *grid.shape), device=DEV, dtype=torch.int32)
    volume = torch.zeros((len(labels), 2), device=DEV, dtype=torch.float64)
    samples, n = [], 0
    for u in steps:
        out = G.native_warp(dev(u), grid, im=dev(im), seg=dev(seg), fill=fill)
        G.label_posterior_update(out['seg'], labels, counts, volume, n)
        samples += list(out['im'][:, 0].cpu().numpy())
        n += u.shape[0]
    return {'counts': counts, 'volume': volume, **dict(zip(IMAGE, welford32(samples)))}


def assert_same(state, want):
    assert torch.equal(state['counts'], want['counts']), 'counts'
    assert torch.equal(state['volume'].view(torch.int64), want['volume'].view(torch.int64)), (state['volume'], want['volume'])
    for key in IMAGE:
        got, ref = state[key].cpu().numpy().view(np.int32), np.asarray(want[key], np.float32).view(np.int32)
        assert np.array_equal(got, ref), f'{key}: {(got != ref).sum()} voxels differ in their bits'


# ---------------------------------------------------------------- 1. against the composition
@pytest.mark.parametrize('shape, dims, C, Cim, bump', [
    ((10, 13, 16), (8, 8, 8), 1, 1, 0.0),
    ((11, 20, 14), (12, 10, 8), 2, 2, 0.0),
    ((33, 40, 37), (16, 16, 16), 2, 1, 0.0),   # 48 840 voxels: no multiple of 64, several blocks, a ragged tail on every axis
    ((11, 20, 14), (12, 10, 8), 2, 1, 0.5),    # + 0.5 on a channel: sources leave the padded box
])
def test_three_steps_against_the_composition(shape, dims, C, Cim, bump):
    grid = NativeGrid.from_shape(shape, dims, (2.0, 1.5, 1.0))
    im, seg = volumes(shape, 3, Cim)
    fill = float(im.min())
    steps = [R.smooth_field(C, dims, 40 + s) for s in range(3)]
    for u in steps:
        u[:, 1] += bump
    state, n = fused(steps, grid, seg, im, fill)
    want = composition(steps, grid, seg, im, fill)
    assert n == 3 * C
    assert_same(state, want)
    assert int(want['counts'][:2].sum()) > 0 and int(want['counts'][2].sum()) == 0     # 7 is absent from the map
    assert int(want['counts'].sum()) < n * int(np.prod(shape))                        # and some voxels are "other"
    if C > 1 or bump:
        assert float(state['m2'].max()) > 0
    if bump:
        # along axis 1, which has no pad here: the border rule repeats the last native row
        assert bool((R.source_coordinate(steps[0], grid)[:, 1].max() > grid.padded[1])), 'no source left the padded box'


def test_the_restatement_agrees_too():
    """the numpy restatement the host tests prove on the exact cases gives the device's counts and the image state's bits on a
    smooth field -- where no label hangs on a tie: the restatement rounds the same float32 coordinate"""
    grid = NativeGrid.from_shape((10, 13, 16), (8, 8, 8))
    im, seg = volumes(grid.shape, 3)
    steps = [R.smooth_field(2, grid.dims, 50 + s) for s in range(2)]
    state, n = fused(steps, grid, seg, im, 0.25)
    ref = NP.native_posterior_np([u.numpy() for u in steps], grid, seg.numpy()[:, 0], LABELS, im.numpy()[:, 0], 0.25)
    assert np.array_equal(state['counts'].cpu().numpy(), ref['counts'])
    assert np.array_equal(state['volume'].cpu().numpy(), np.stack([ref['vol_mean'], ref['vol_m2']], 1))
    for key in IMAGE:
        assert np.array_equal(state[key].cpu().numpy().view(np.int32), ref[key].view(np.int32)), key


# ---------------------------------------------------------------- 2. the exact cases, on the device
@pytest.mark.parametrize('shape, dims', [((10, 13, 16), (8, 8, 8)), ((6, 7, 5), (16, 16, 16))])
@pytest.mark.parametrize('C', [1, 3])
def test_zero_field(shape, dims, C):
    grid = NativeGrid.from_shape(shape, dims)
    im, seg = volumes(shape, 6)
    state, n = fused([torch.zeros(C, 3, *dims)], grid, seg, im, float(im.min()))
    lab = torch.tensor(LABELS).view(-1, 1, 1, 1)
    hit = (seg[0] == lab).to(torch.int32)
    assert torch.equal(state['counts'].cpu(), C * hit)
    assert torch.equal(state['volume'].cpu(), torch.stack([hit.sum((1, 2, 3)).double(), torch.zeros(3, dtype=torch.float64)], 1))
    assert torch.equal(bits(state['mean'].cpu()), bits(im[0, 0])) and not state['m2'].any()
    assert torch.equal(state['low'].cpu(), im[0, 0]) and torch.equal(state['high'].cpu(), im[0, 0])


@pytest.mark.parametrize('per_channel, shift', SHIFTS)
def test_integer_translations(per_channel, shift):
    im, seg, _ = R.random_volumes(DYADIC.shape, 5)
    fill = float(im.min())
    state, n = fused([R.constant_field(2, DYADIC.dims, per_channel)], DYADIC, seg, im, fill)
    seg_want, im_want = R.shifted(seg, DYADIC, shift, 0)[0, 0], R.shifted(im, DYADIC, shift, fill)[0, 0]
    hit = (seg_want == torch.tensor(LABELS).view(-1, 1, 1, 1)).to(torch.int32)
    assert torch.equal(state['counts'].cpu(), 2 * hit)
    assert torch.equal(state['volume'][:, 0].cpu(), hit.sum((1, 2, 3)).double()) and not state['volume'][:, 1].any()
    for key in ('mean', 'low', 'high'):
        assert torch.equal(bits(state[key].cpu()), bits(im_want)), key
    assert not state['m2'].any()


# ---------------------------------------------------------------- 3. instantiations, determinism, the first record
def smooth_case(C=2, Cim=1):
    grid = NativeGrid.from_shape((33, 40, 37), (16, 16, 16))
    im, seg = volumes(grid.shape, 9, Cim)
    return grid, im, seg, [R.smooth_field(C, grid.dims, 60 + s) for s in range(2)]


def test_the_parts_alone_give_the_bits_of_the_combined_launch():
    grid, im, seg, steps = smooth_case()
    both, _ = fused(steps, grid, seg, im, 0.0)
    labels_only, _ = fused(steps, grid, seg=seg)
    image_only, _ = fused(steps, grid, im=im, fill=0.0)
    assert sorted(labels_only) == ['counts', 'labels', 'volume'] and sorted(image_only) == sorted(IMAGE)
    assert torch.equal(labels_only['counts'], both['counts']) and torch.equal(labels_only['volume'], both['volume'])
    for key in IMAGE:
        assert torch.equal(bits(image_only[key]), bits(both[key])), key
    default_fill, _ = fused(steps, grid, im=im)   # the default fill is the image's minimum
    explicit, _ = fused(steps, grid, im=im, fill=float(im.min()))
    assert all(torch.equal(bits(default_fill[k]), bits(explicit[k])) for k in IMAGE)


def test_two_identical_call_sequences_are_bit_identical():
    grid, im, seg, steps = smooth_case(Cim=2)
    a, _ = fused(steps, grid, seg, im, 0.0)
    b, _ = fused(steps, grid, seg, im, 0.0)
    assert torch.equal(a['counts'], b['counts']) and torch.equal(a['volume'].view(torch.int64), b['volume'].view(torch.int64))
    assert all(torch.equal(bits(a[k]), bits(b[k])) for k in IMAGE)


def test_the_first_record_overwrites_a_poisoned_image_state():
    grid, im, seg, steps = smooth_case()
    clean, _ = fused(steps, grid, seg, im, 0.0)
    state = P.native_posterior_state(grid, LABELS, True, DEV)
    for key in IMAGE:
        state[key].fill_(float('nan'))
    state['volume'].fill_(float('nan'))
    poisoned, _ = fused(steps, grid, seg, im, 0.0, state=state)
    assert all(torch.equal(bits(clean[k]), bits(poisoned[k])) for k in IMAGE)
    assert torch.equal(clean['volume'], poisoned['volume'])
    # and a later call continues: two steps in one sequence == one step, then one more with records_before = C
    first, n = fused(steps[:1], grid, seg, im, 0.0)
    second, _ = fused(steps[1:], grid, seg, im, 0.0, state=first, records_before=n)
    assert torch.equal(second['counts'], clean['counts']) and all(torch.equal(bits(second[k]), bits(clean[k])) for k in IMAGE)


# ---------------------------------------------------------------- 4. refusals
def abi_case():
    """arguments of irs_native_posterior_update that pass, on real buffers, with a sentinel in every output"""
    grid = NativeGrid.from_shape((6, 7, 5), (4, 4, 4))
    C, K = 2, 2
    i3 = lambda v: (ctypes.c_int32 * 3)(*v)
    t = {'displacement': torch.zeros(C, 3, 4, 4, 4, device=DEV), 'im': torch.ones(1, 1, 6, 7, 5, device=DEV),
         'seg': torch.ones(1, 1, 6, 7, 5, device=DEV, dtype=torch.int16),
         'counts': torch.full((K, 6, 7, 5), 77, device=DEV, dtype=torch.int32),
         'volume': torch.full((K, 2), 77.0, device=DEV, dtype=torch.float64),
         **{k: torch.full((6, 7, 5), 77.0, device=DEV) for k in IMAGE}, 'ws': torch.zeros(1 << 16, device=DEV, dtype=torch.uint8)}
    p = {k: ctypes.c_void_p(v.data_ptr()) for k, v in t.items()}
    need = ctypes.c_size_t()
    assert L.load().irs_native_posterior_workspace(C, K, i3(grid.shape), ctypes.byref(need)) == 0 and 16 <= need.value <= 1 << 16
    good = dict(displacement=p['displacement'], C=C, dims=i3(grid.dims), native=i3(grid.shape), padding=i3(grid.padding), im=p['im'],
                seg=p['seg'], Cim=1, fill=0.0, labels=(ctypes.c_int32 * K)(1, 2), K=K, counts=p['counts'], volume=p['volume'],
                mean=p['mean'], m2=p['m2'], low=p['low'], high=p['high'], records_before=0, ws=p['ws'], ws_bytes=need.value, stream=None)
    return t, good, need.value, i3


I32MAX = 2 ** 31 - 1
REFUSALS = [
    ('displacement=null', dict(displacement=None), 'bad arguments'),
    ('ws=null', dict(ws=None), 'bad arguments'),
    ('C=0', dict(C=0), 'C = 0 chains, 1..8'),
    ('C=9', dict(C=9), 'C = 9 chains, 1..8'),
    ('Cim=3', dict(Cim=3), 'moving volumes of 3 chains, 1 or 2 needed'),
    ('native=1', dict(native=(6, 1, 5)), 'native[1] = 1 < 2'),
    ('padding<0', dict(padding=(0, -1, 0)), 'padding[1] = -1 < 0'),
    ('dims=1', dict(dims=(4, 1, 4)), 'dims[1] = 1 < 2'),
    ('K=0', dict(K=0), '1..64 labels in the int16 range'),
    ('K=65', dict(K=65), '1..64 labels in the int16 range'),
    ('label-range', dict(labels=(1, 40000)), '1..64 labels in the int16 range'),
    ('label-twice', dict(labels=(2, 2)), 'label 2 appears twice'),
    ('seg-alone', dict(counts=None), 'seg, labels, counts and volume go together, 3 of them given'),
    ('labels-missing', dict(labels=None), 'seg, labels, counts and volume go together, 3 of them given'),
    ('im-alone', dict(mean=None, low=None), 'im, mean, m2, low and high go together, 3 of them given'),
    ('nothing', dict(seg=None, labels=None, counts=None, volume=None, im=None, mean=None, m2=None, low=None, high=None),
     'neither the label nor the image part is given'),
    ('records=-1', dict(records_before=-1), 'records_before = -1 < 0'),
    ('records=ceiling', dict(records_before=I32MAX - 1), f'{I32MAX - 1} records + 2 chains overflow the int32 record count'),
    ('fill=nan', dict(fill=float('nan')), 'fill = nan, a finite value needed'),
    ('fill=inf', dict(fill=float('inf')), 'fill = inf, a finite value needed'),
    ('ws-1', dict(ws_bytes=-1), 'needed (irs_native_posterior_workspace)'),
]


@pytest.mark.parametrize('case, replaced, message', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_abi_refusals_launch_nothing(case, replaced, message):
    t, good, need, i3 = abi_case()
    args = dict(good)
    for k, v in replaced.items():
        args[k] = (i3(v) if k in ('native', 'padding', 'dims') else (ctypes.c_int32 * len(v))(*v) if k == 'labels' and v is not None
                   else need - 1 if k == 'ws_bytes' else v)
    lib = L.load()
    assert lib.irs_native_posterior_update(*args.values()) != 0, case
    assert message in lib.irs_last_error().decode(), lib.irs_last_error().decode()
    torch.cuda.synchronize()
    assert all(bool((t[k] == 77).all()) for k in ('counts', 'volume', *IMAGE)), 'a refused call wrote to the state'


def test_the_good_abi_call_and_the_workspace_query():
    t, good, need, i3 = abi_case()
    lib = L.load()
    assert lib.irs_native_posterior_update(*good.values()) == 0, lib.irs_last_error().decode()
    torch.cuda.synchronize()
    assert bool((t['counts'][0] == 77 + 2).all()) and bool((t['counts'][1] == 77).all()) and bool((t['mean'] == 1).all())
    nbytes = ctypes.c_size_t()
    for bad in (dict(C=0), dict(K=-1), dict(K=65), dict(native=(6, 1, 5))):
        a = {'C': 2, 'K': 2, 'native': (6, 7, 5), **bad}
        assert lib.irs_native_posterior_workspace(a['C'], a['K'], i3(a['native']), ctypes.byref(nbytes)) != 0, bad
    assert lib.irs_native_posterior_workspace(2, 2, i3((6, 7, 5)), None) != 0
    assert lib.irs_native_posterior_workspace(2, 0, i3((6, 7, 5)), ctypes.byref(nbytes)) == 0 and nbytes.value >= 16


def test_python_refusals():
    grid = NativeGrid.from_shape((6, 7, 5), (4, 4, 4))
    u = torch.zeros(2, 3, 4, 4, 4, device=DEV)
    im, seg = torch.zeros(1, 1, 6, 7, 5, device=DEV), torch.zeros(1, 1, 6, 7, 5, device=DEV, dtype=torch.int16)
    both = lambda: P.native_posterior_state(grid, [1, 2], True, DEV)
    with pytest.raises(L.IrsError, match='neither labels nor image'):
        P.native_posterior_state(grid, None, False, DEV)
    with pytest.raises(L.IrsError, match='extents of at least 2'):
        P.native_posterior_state(NativeGrid.from_shape((6, 1, 5), (4, 4, 4)), [1], False, DEV)
    with pytest.raises(L.IrsError, match='not on the registration grid'):
        P.native_posterior_update(u[..., :3].contiguous(), grid, both(), 0, seg=seg, im=im, fill=0.0)
    with pytest.raises(L.IrsError, match='seg and the counts'):
        P.native_posterior_update(u, grid, both(), 0, im=im, fill=0.0)
    with pytest.raises(L.IrsError, match='im and the mean'):
        P.native_posterior_update(u, grid, both(), 0, seg=seg)
    with pytest.raises(L.IrsError, match='seg must be torch.int16'):
        P.native_posterior_update(u, grid, both(), 0, seg=seg.int(), im=im, fill=0.0)
    with pytest.raises(L.IrsError, match='does not match the native grid'):
        P.native_posterior_update(u, grid, both(), 0, seg=seg, im=im[..., :4].contiguous(), fill=0.0)
    with pytest.raises(L.IrsError, match='share their leading size'):
        P.native_posterior_update(u, grid, both(), 0, seg=seg.expand(2, -1, -1, -1, -1).contiguous(), im=im, fill=0.0)
    with pytest.raises(L.IrsError, match='fill must be finite'):
        P.native_posterior_update(u, grid, both(), 0, seg=seg, im=im, fill=float('nan'))
    state = both()
    state['counts'] = state['counts'][:1]
    with pytest.raises(L.IrsError, match='counts must be a'):
        P.native_posterior_update(u, grid, state, 0, seg=seg, im=im, fill=0.0)
    state = both()
    del state['m2']
    with pytest.raises(L.IrsError, match='image part of the state must hold'):
        P.native_posterior_update(u, grid, state, 0, seg=seg, im=im, fill=0.0)
    with pytest.raises(L.IrsError, match='records_before = -1'):
        P.native_posterior_update(u, grid, both(), -1, seg=seg, im=im, fill=0.0)
    with pytest.raises(L.IrsError, match='appears twice'):
        P.native_posterior_update(u, grid, P.native_posterior_state(grid, [1, 1], False, DEV), 0, seg=seg)
    with pytest.raises(L.IrsError, match='GPU only'):
        P.native_posterior_update(u.cpu(), grid, both(), 0, seg=seg, im=im, fill=0.0)


# ---------------------------------------------------------------- 5. the finalize on the native extents
def test_finalize_gives_mm3_under_the_zooms():
    zooms = (2.0, 1.5, 1.0)
    grid = NativeGrid.from_shape((11, 20, 14), (12, 10, 8), zooms)
    im, seg = volumes(grid.shape, 3)
    im_fixed, seg_fixed = volumes(grid.shape, 4)
    mask = torch.rand(grid.shape, generator=torch.Generator().manual_seed(1)) > 0.2
    steps = [R.smooth_field(2, grid.dims, 70 + s) for s in range(3)]
    names = {'one': 1, 'three': 3, 'seven': 7}
    maps, rec = calc_native_posterior([dev(u) for u in steps], grid, seg, names, im, float(im.min()), seg_fixed[0, 0], im_fixed[0, 0],
                                      mask, 0.05)
    want = composition(steps, grid, seg, im, float(im.min()))
    assert rec.records == 6 and torch.equal(rec.state['counts'], want['counts'])
    # the existing finalizers on the composition's state, on the native extents
    entropy, map_label, raw, ms = G.label_posterior_finalize(want['counts'], 6, LABELS, dev(seg_fixed[0, 0]), dev(mask))
    assert torch.equal(maps['labels']['entropy'], entropy) and torch.equal(maps['labels']['map'], map_label)
    voxels = label_summary(raw.cpu().numpy(), want['volume'].cpu().numpy(), 6, ms.cpu().numpy(), list(names), (1.0, 1.0, 1.0))
    s = maps['labels']['summary']
    for name in names:
        for key in ('vol_mean', 'vol_std', 'uncertain_vol'):   # mm^3: the voxel counts times the zoom product 3.0
            assert s['structures'][name][key] == voxels['structures'][name][key] * 3.0, (name, key)
        for key in ('soft_DSC', 'DSC_MAP', 'ECE'):
            a, b = s['structures'][name][key], voxels['structures'][name][key]
            assert a == b or (a != a and b != b), (name, key)
    assert s['structures']['one']['vol_mean'] > 0 and s['structures']['seven']['vol_mean'] == 0
    assert s['voxels'] == int(mask.sum()) and s['entropy_mean'] == voxels['entropy_mean']
    assert torch.equal(rec.probabilities(), want['counts'].float() / 6)
    # the image part: image_posterior_finalize on the composition's state
    from ir_sgmcmc_amd.image_posterior import image_posterior_finalize
    state = {k: dev(torch.from_numpy(np.asarray(want[k]))).unsqueeze(0) for k in IMAGE}
    std, rng, z, isum, fsum = image_posterior_finalize(state, 0, 6, dev(im_fixed[0, 0]), 0.05, dev(mask))
    for key, ref in (('std', std), ('range', rng), ('z', z), ('mean', state['mean'][0])):
        assert torch.equal(bits(maps['image'][key]), bits(ref)), key
    assert maps['image']['summary']['voxels'] == int(mask.sum()) and maps['image']['summary']['std_max'] > 0


# ---------------------------------------------------------------- 6. the trainer
NATIVE, ZOOMS, N = (12, 15, 13), (1.0, 1.5, 2.0), 8


def make_trainer(tmp_path, data_dir, **trainer_over):
    cfg = json.load(open(os.path.join(ROOT, 'configs', 'synthetic_gmm_lognormal.json')))
    cfg['trainer']['save_dir'] = str(tmp_path)
    cfg['data_loader'] = {'type': 'BiobankDataLoader', 'args': {'data_dir': data_dir, 'dims': [N, N, N], 'sigma_v_init': 0.5,
                                                                 'u_v_init': 0.1}}
    cfg['trainer'].update(trainer_over)
    config = ConfigParser.from_dict(copy.deepcopy(cfg), timestamp='t')
    dl = config.init_data_loader()
    losses = config.init_losses()
    tm, rm = config.init_transformation_and_registration_modules()
    return Trainer(config, dl, losses, tm, rm, config.init_metrics(), device=DEV)


def test_trainer_native_posterior(tmp_path, monkeypatch):
    data_dir = R.write_pair(tmp_path / 'data', NATIVE, ZOOMS)
    kw = dict(no_chains=2, no_iters_burn_in=2, no_samples_MCMC=8, log_period_MCMC=4, checkpoint_period=6, native_resolution=True)
    on_kw = dict(kw, native_posterior={'period': 2, 'prob_maps': True, 'std_floor': 0.01})
    seen = []   # the displacements the recorder took, in voxels of the registration grid
    update = NativePosterior._update
    monkeypatch.setattr(NativePosterior, '_update', lambda self, d: (seen.append(d.detach().clone()), update(self, d))[1])
    torch.manual_seed(0)
    a = make_trainer(tmp_path / 'a', data_dir, **on_kw)
    a.run()
    assert len(seen) == 4 and a._native_posterior.records == 8   # samples 4, 6, 8, 10 of two chains
    taken = list(seen)
    grid = NativeGrid.from_shape(NATIVE, (N, N, N), ZOOMS)
    pair = a.data_loader.native()
    up = lambda t: t.unsqueeze(0)
    maps, rec = calc_native_posterior(taken, grid, up(pair['moving']['seg']), a.structures_dict, up(pair['moving']['im']),
                                      pair['fill']['moving'], pair['fixed']['seg'][0], pair['fixed']['im'][0], pair['fixed']['mask'][0],
                                      0.01, voxels=True)
    assert all(torch.equal(bits(a._native_posterior.state[k]), bits(rec.state[k])) for k in ('counts', *IMAGE))
    # the files: native shape, header zooms, the recomputed maps
    folder = a.config.save_dirs['samples']
    read = lambda name, dtype=np.float32: read_nifti(str(folder / name), dtype)
    expected = {'MCMC_seg_entropy_native.nii.gz': maps['labels']['entropy'], 'MCMC_seg_MAP_native.nii.gz': maps['labels']['map'],
                **{f'MCMC_seg_prob_{s}_native.nii.gz': p for s, p in zip(a.structures_dict, rec.probabilities())},
                **{f'MCMC_im_moving_{k}_native.nii.gz': torch.nan_to_num(maps['image'][k], nan=0.0) for k in ('mean', 'std', 'range', 'z')}}
    for name, want in expected.items():
        arr, zooms = read(name, np.int16 if 'MAP' in name else np.float32)
        assert arr.shape == NATIVE and zooms == ZOOMS and (arr == want.cpu().numpy()).all(), name
    assert float(maps['image']['std'].max()) > 0 and int(rec.state['counts'].sum()) > 0
    # the metrics: exactly the keys of the option, the volumes in mm^3 under the header zooms
    res = a.metrics.result()
    new = native_posterior_metric_names(a.native_posterior_options, a.structures_dict)
    assert sorted(k for k in res if k.startswith('MCMC/native/')) == sorted(new) and len(new) == 15 * 6 + 3 + 6
    s = maps['labels']['summary']
    for name, st in s['structures'].items():
        for key, value in st.items():
            got = res[f'MCMC/native/seg/{key}/{name}']
            assert got == value or (got != got and value != value), (name, key)
    thalamus = s['structures']['left_thalamus']   # label 10 of the synthetic pair
    assert thalamus['vol_mean'] == float(rec.state['volume'][0, 0]) * 3.0 > 0
    assert json.dumps(a.native_posterior_summary['labels']['structures']) == json.dumps(s['structures'])   # (NaN compares as text)
    assert all(res[f'MCMC/native/image/moving/{k}'] == maps['image']['summary'][k] for k in ('std_mean', 'std_max', 'range_max', 'z_rms'))
    # resumed from the checkpoint in the middle of the recording, the state and the summary come out bit for bit
    ck = a.config.save_dirs['checkpoints'] / 'checkpoint_0000006.pt'
    sd = torch.load(ck, map_location='cpu', weights_only=True)
    assert sd['native_posterior']['records'] == 4 and tuple(sd['native_posterior']['counts'].shape) == (15, *NATIVE)
    torch.manual_seed(0)
    b = make_trainer(tmp_path / 'b', data_dir, resume=str(ck), **on_kw)
    b.run()
    assert all(torch.equal(bits(a._native_posterior.state[k]), bits(b._native_posterior.state[k])) for k in ('counts', *IMAGE))
    assert torch.equal(a._native_posterior.state['volume'], b._native_posterior.state['volume'])
    strip = lambda summary: json.dumps({p: {k: v for k, v in s.items() if k != 'raw'} for p, s in summary.items()}, sort_keys=True)
    assert strip(a.native_posterior_summary) == strip(b.native_posterior_summary)
    assert torch.equal(bits(a.v_curr_state), bits(b.v_curr_state))
    del sd['native_posterior']
    torch.save(sd, tmp_path / 'without.pt')
    with pytest.raises(ValueError, match='native_posterior'):
        make_trainer(tmp_path / 'c', data_dir, resume=str(tmp_path / 'without.pt'), **on_kw).run()
    # with the option off: the same chain, the same metric keys, files and checkpoint keys as without the feature
    torch.manual_seed(0)
    off = make_trainer(tmp_path / 'off', data_dir, **kw)
    off.run()
    assert torch.equal(bits(off.v_curr_state), bits(a.v_curr_state)) and torch.equal(bits(off.displacement_mean), bits(a.displacement_mean))
    off_keys = list(off.metrics.result())
    assert [k for k in res if k not in new] == off_keys and not [k for k in off_keys if k.startswith('MCMC/native/')]
    assert off.native_posterior_options is None and off._native_posterior is None and off.native_posterior_summary is None
    assert 'fixed_im' not in off._native and 'fixed_mask' not in off._native
    names = lambda tr: sorted(p.name for p in tr.config.save_dirs['samples'].iterdir())
    assert names(a) == sorted(names(off) + list(expected))
    sd_off = torch.load(off.config.save_dirs['checkpoints'] / 'checkpoint_0000006.pt', map_location='cpu', weights_only=True)
    assert set(sd_off) == set(sd)


def test_trainer_refuses_the_option_without_the_native_pair(tmp_path):
    data_dir = R.write_pair(tmp_path / 'data', NATIVE, ZOOMS)
    with pytest.raises(ValueError, match='needs trainer.native_resolution'):
        make_trainer(tmp_path / 'a', data_dir, native_posterior=True)
