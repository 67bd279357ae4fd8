"""Intensity similarity on the GPU (ops.image_similarity, utils.calc_image_similarity, the trainer's `image_similarity` option)
against the numpy restatement of tests/_image_similarity.py, which shares no code with the HIP path.

The histogram and the three counts are integers and must be EQUAL: the binning is stated in float32 operations that numpy
repeats bit for bit.  The float columns: the sums are double sums of at most 2e4 non-negative terms, which order and FMA
contraction move by at most n 2^-53 = 2e-12 relative; NCC's cancellation amplifies that by sum f^2 / (n var) = 4 for uniform
images; the entropies are at most 128^2 terms of p ln p from exact counts with a log good to a few ulp.  The bounds -- MSE 1e-9
relative, everything else 1e-9 absolute -- leave two to three orders of margin (the restatement summed in a permuted order
differs from itself by 6e-14 for MSE and 2e-13 for NCC)."""
import copy
import json
import math
import os

import numpy as np
import pytest
import torch

from ir_sgmcmc_amd import _lib as L
from ir_sgmcmc_amd import ops
from ir_sgmcmc_amd.utils import calc_image_similarity
from tests import _image_similarity as S
from tests._report import check

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = (0.0, 1.0)
COL = {k: j for j, k in enumerate(S.COLUMNS)}

ODD, VEC, BIG = (5, 7, 9), (4, 8, 16), (17, 16, 65)  # 315 voxels (scalar path); the 16-byte path; 17 680: several blocks per chain
# (shape, C, Cf, mask, bins, spoiled): every value of every axis appears; BIG meets 128 bins and two chains
SWEEP = [(ODD, 1, 1, None, 2, False), (ODD, 2, 1, 'bool', 37, False), (ODD, 2, 2, 'uint8', 64, False),
         (ODD, 2, 2, 'bool', 128, True), (VEC, 1, 1, 'bool', 128, False), (VEC, 2, 2, None, 37, False),
         (VEC, 2, 1, 'uint8', 2, False), (BIG, 2, 1, 'bool', 128, False), (BIG, 2, 2, None, 64, False),
         (BIG, 1, 1, 'uint8', 37, False), (BIG, 2, 2, 'bool', 128, True)]


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def gpu(fixed, moving, mask=None, bins=64, fr=UNIT, mr=UNIT, want_hist=True):
    out = ops.image_similarity(dev(fixed), dev(moving), dev(mask), bins, fr, mr, want_hist=want_hist)
    return {k: v.cpu().numpy() for k, v in out.items()}


def build(shape, C, Cf, mask, spoiled, seed):
    fixed, moving = S.random_pair(shape, C, Cf, seed)
    if spoiled:
        fixed, moving = S.spoil(fixed, moving, seed + 1)
    m = None if mask is None else S.random_mask(shape, seed + 2, bool if mask == 'bool' else np.uint8)
    if spoiled:  # most of the spoiled voxels inside the mask, the first plane outside it
        m = np.ones_like(m)
        m[:, :, 0] = 0
    return fixed, moving, m


def compare(name, got, hist, stats):
    """integers equal; MSE to 1e-9 relative, the other float columns to 1e-9 absolute; NaN where the restatement has NaN"""
    assert got['hist'].dtype == np.int32 and got['stats'].dtype == np.float64
    assert (got['hist'] == hist).all(), name
    assert (got['stats'][:, :3] == stats[:, :3]).all(), (name, got['stats'][:, :3], stats[:, :3])
    assert (np.isnan(got['stats']) == np.isnan(stats)).all(), (name, got['stats'], stats)
    ok = ~np.isnan(stats[:, COL['mse']])
    check('image_similarity', 'mse_relative', got['stats'][ok, COL['mse']] / stats[ok, COL['mse']], np.ones(int(ok.sum())), 1e-9)
    for k in S.COLUMNS[4:]:
        ok = ~np.isnan(stats[:, COL[k]])
        check('image_similarity', k, got['stats'][ok, COL[k]], stats[ok, COL[k]], 1e-9)


@pytest.mark.parametrize('shape,C,Cf,mask,bins,spoiled', SWEEP)
def test_against_the_restatement(shape, C, Cf, mask, bins, spoiled):
    fixed, moving, m = build(shape, C, Cf, mask, spoiled, seed=len(shape) + C + bins)
    hist, stats = S.reference(fixed, moving, m, bins, UNIT, UNIT)
    got = gpu(fixed, moving, m, bins)
    assert got['hist'].shape == (C, bins, bins) and got['stats'].shape == (C, L.IRS_SIMILARITY_STATS)
    if spoiled:
        assert (stats[:, COL['n_nonfinite']] > 0).all() and (stats[:, COL['n_clipped']] > 0).all()
    else:
        assert stats[0, COL['n']] > 100 and (stats[:, 1:3] == 0).all()
    compare(f'{shape} C={C} Cf={Cf} {mask} bins={bins}', got, hist, stats)


def test_ranges_taken_from_the_images_and_unaligned_bases():
    fixed, moving, m = build(VEC, 2, 2, 'bool', False, seed=5)
    fixed, moving = fixed * np.float32(3.0) - np.float32(1.0), moving * np.float32(0.5)
    fr, mr = (float(fixed.min()), float(fixed.max())), (float(moving.min()), float(moving.max()))
    hist, stats = S.reference(fixed, moving, m, 32, fr, mr)
    out = ops.image_similarity(dev(fixed), dev(moving), dev(m), 32, want_hist=True)
    compare('ranges from the images', {k: v.cpu().numpy() for k, v in out.items()}, hist, stats)
    assert stats[:, COL['n_clipped']].sum() == 0  # the maximum itself lands in the last bin, unclipped
    rows = calc_image_similarity(dev(fixed), dev(moving), dev(m), 32)
    assert [list(r) for r in rows] == [list(S.COLUMNS)] * 2
    assert [[r[k] for k in S.COLUMNS[:3]] for r in rows] == stats[:, :3].astype(int).tolist() and isinstance(rows[0]['n'], int)
    assert [r['mi'] for r in rows] == out['stats'][:, COL['mi']].tolist()
    # V % 4 == 0 but bases 4 bytes off a 16-byte boundary: the scalar path
    V = int(np.prod(VEC))
    buf_f, buf_m = torch.zeros(2 * V + 1, device=DEV), torch.zeros(2 * V + 1, device=DEV)
    buf_f[1:] = dev(fixed).reshape(-1)
    buf_m[1:] = dev(moving).reshape(-1)
    off = ops.image_similarity(buf_f[1:].view(2, 1, *VEC), buf_m[1:].view(2, 1, *VEC), dev(m), 32, fr, mr, want_hist=True)
    assert buf_f[1:].data_ptr() % 16 == 4 and torch.equal(off['hist'], out['hist'])
    compare('unaligned bases', {k: v.cpu().numpy() for k, v in off.items()}, hist, stats)


# ---------------------------------------------------------------- known answers (proved on the host: test_image_similarity_host.py)
def test_identical_images():
    f, _ = S.random_pair(BIG, 2, 2, seed=11)
    got = gpu(f, f, None, 64)
    for c in range(2):
        h = got['hist'][c]
        assert h.sum() == f[c].size and np.count_nonzero(h - np.diag(np.diag(h))) == 0
    st = got['stats']
    assert (st[:, COL['mse']] == 0.0).all() and (st[:, COL['n']] == f[0].size).all()
    assert np.abs(st[:, COL['nmi']] - 2.0).max() <= 1e-9 and np.abs(st[:, COL['mi']] - st[:, COL['h_fixed']]).max() <= 1e-9
    assert np.abs(st[:, COL['ncc']] - 1.0).max() <= 1e-9


def test_independent_lattice():
    f, m = S.lattice(8, 5)
    got = gpu(f.reshape(1, 1, 5, 8, 8), m.reshape(1, 1, 5, 8, 8), None, 8)
    assert (got['hist'] == 5).all()
    st = got['stats'][0]
    assert st[COL['n']] == 320 and st[COL['n_clipped']] == 0
    assert abs(st[COL['mi']]) <= 1e-9 and abs(st[COL['h_fixed']] - math.log(8)) <= 1e-9 and abs(st[COL['nmi']] - 1.0) <= 1e-9


def test_bin_edges_under_a_mask_of_eight_voxels():
    shape = (3, 4, 5)
    f, m = S.random_pair(shape, 1, 1, seed=2)
    mask = np.zeros((1, 1, *shape), bool)
    where = [0, 7, 13, 22, 31, 38, 44, 59]
    f.reshape(-1)[where] = S.EDGE_VALUES
    m.reshape(-1)[where] = np.float32(0.5)
    mask.reshape(-1)[where] = True
    got = gpu(f, m, mask, 8)
    want = np.zeros((8, 8), np.int64)
    for b in S.EDGE_BINS:
        want[b, 4] += 1
    assert (got['hist'][0] == want).all()
    assert got['stats'][0, :3].tolist() == [8.0, 0.0, 2.0]
    # and on the moving side
    got = gpu(m, f, mask, 8)
    assert (got['hist'][0] == want.T).all() and got['stats'][0, :3].tolist() == [8.0, 0.0, 2.0]


# ---------------------------------------------------------------- constant images, the empty mask
def test_constant_images_and_the_empty_mask():
    """every voxel in one joint bin: the worst case for same-address adds"""
    V = int(np.prod(BIG))
    f = np.full((1, 1, *BIG), 0.5, np.float32)
    m = np.full((2, 1, *BIG), 0.25, np.float32)
    for aggregate in (None, 0):  # the default -- one add per wavefront here -- and plain atomics
        if aggregate is not None:
            L.option_set('similarity_aggregate', aggregate)
        try:
            got = gpu(f, m, None, 64)
        finally:
            L.option_set('similarity_aggregate', 1)
        for c in range(2):
            assert got['hist'][c, 32, 16] == V == got['hist'][c].sum()
        st = got['stats']
        assert (st[:, COL['n']] == V).all() and (st[:, COL['mse']] == 0.0625).all() and (st[:, COL['h_joint']] == 0.0).all()
        assert np.isnan(st[:, COL['ncc']]).all() and np.isnan(st[:, COL['nmi']]).all() and (st[:, COL['mi']] == 0.0).all()
    half = S.random_mask(BIG, 41)  # wavefronts with one bin but not every lane in the mask
    got = gpu(f, m, half, 64)
    assert (got['hist'][:, 32, 16] == half.sum()).all() and (got['hist'].sum(axis=(1, 2)) == half.sum()).all()
    assert (got['stats'][:, COL['n']] == half.sum()).all()
    got = gpu(f, m, np.zeros((1, 1, *BIG), bool), 64)
    assert not got['hist'].any() and (got['stats'][:, :3] == 0).all() and np.isnan(got['stats'][:, 3:]).all()


# ---------------------------------------------------------------- symmetry, reproducibility
def test_swapping_the_images_transposes_the_histogram():
    fixed, moving, m = build(BIG, 2, 2, 'bool', False, seed=21)
    fr, mr = (0.0, 1.0), (-0.1, 1.2)
    a, b = gpu(fixed, moving, m, 37, fr, mr), gpu(moving, fixed, m, 37, mr, fr)
    assert (a['hist'] == b['hist'].transpose(0, 2, 1)).all() and not (a['hist'] == b['hist']).all()
    sa, sb = a['stats'], b['stats']
    assert (sa[:, COL['h_fixed']] == sb[:, COL['h_moving']]).all() and (sa[:, COL['h_moving']] == sb[:, COL['h_fixed']]).all()
    assert (sa[:, :3] == sb[:, :3]).all() and (sa[:, COL['mse']] == sb[:, COL['mse']]).all()
    for k in ('ncc', 'h_joint', 'mi', 'nmi'):
        assert np.abs(sa[:, COL[k]] - sb[:, COL[k]]).max() <= 1e-9, k


def test_two_identical_calls_are_bit_identical():
    fixed, moving, m = build(BIG, 2, 1, 'uint8', False, seed=31)
    f, mv, mk = dev(fixed), dev(moving), dev(m)
    a = ops.image_similarity(f, mv, mk, 128, UNIT, UNIT, want_hist=True)
    b = ops.image_similarity(f, mv, mk, 128, UNIT, UNIT, want_hist=True)
    c = ops.image_similarity(f, mv, mk, 128, UNIT, UNIT)
    bits = lambda t: t.view(torch.int64)
    assert torch.equal(a['hist'], b['hist']) and torch.equal(bits(a['stats']), bits(b['stats']))
    assert set(c) == {'stats'} and torch.equal(bits(a['stats']), bits(c['stats']))
    # the two forms of the LDS add (one per single-bin wavefront, plain atomics) count the same voxels
    L.option_set('similarity_aggregate', 0)
    try:
        d = ops.image_similarity(f, mv, mk, 128, UNIT, UNIT, want_hist=True)
    finally:
        L.option_set('similarity_aggregate', 1)
    assert torch.equal(a['hist'], d['hist']) and torch.equal(bits(a['stats']), bits(d['stats']))


# ---------------------------------------------------------------- refusals
def test_refusals():
    f, mv = torch.rand(1, 1, *VEC, device=DEV), torch.rand(2, 1, *VEC, device=DEV)
    ok = dict(fixed_range=UNIT, moving_range=UNIT)
    assert ops.image_similarity(f, mv, **ok)['stats'].shape == (2, 10)
    for bins in (1, 129, 64.0):
        with pytest.raises(L.IrsError):
            ops.image_similarity(f, mv, bins=bins, **ok)
    for r in ((1.0, 1.0), (1.0, 0.5), (0.0, float('nan')), (float('-inf'), 1.0)):
        with pytest.raises(L.IrsError):
            ops.image_similarity(f, mv, fixed_range=r, moving_range=UNIT)
        with pytest.raises(L.IrsError):
            ops.image_similarity(f, mv, fixed_range=UNIT, moving_range=r)
    with pytest.raises(L.IrsError):  # Cf = 3 with C = 2
        ops.image_similarity(torch.rand(3, 1, *VEC, device=DEV), mv, **ok)
    with pytest.raises(L.IrsError):
        ops.image_similarity(f.double(), mv, **ok)
    with pytest.raises(L.IrsError):
        ops.image_similarity(f, mv.double(), **ok)
    with pytest.raises(L.IrsError):
        ops.image_similarity(f.cpu(), mv, **ok)
    with pytest.raises(L.IrsError):
        ops.image_similarity(f, mv.cpu(), **ok)
    for mask in (torch.ones(1, 1, 4, 8, 15, dtype=torch.bool, device=DEV), torch.ones(2, 1, *VEC, dtype=torch.bool, device=DEV),
                 torch.ones(*VEC, dtype=torch.bool, device=DEV), torch.ones(1, 1, *VEC, device=DEV)):
        with pytest.raises(L.IrsError):
            ops.image_similarity(f, mv, mask, **ok)
    with pytest.raises(L.IrsError):
        ops.image_similarity(f, mv[:, 0], **ok)
    # a constant image has no range of its own
    with pytest.raises(L.IrsError):
        ops.image_similarity(torch.ones_like(f), mv)


# ---------------------------------------------------------------- trainer
class WithoutSegmentations:
    """the synthetic pair as most clinical pairs come: images and masks only"""

    def __init__(self, loader):
        self.loader = loader

    def __getattr__(self, name):
        return getattr(self.loader, name)

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for fixed, moving, var_params in self.loader:
            yield ({k: v for k, v in fixed.items() if k != 'seg'}, {k: v for k, v in moving.items() if k != 'seg'}, var_params)


def make_trainer(tmp_path, wrap=None, **trainer_over):
    from ir_sgmcmc_amd.parse_config import ConfigParser
    from ir_sgmcmc_amd.trainer import Trainer
    cfg = json.load(open(os.path.join(ROOT, 'configs', 'synthetic_gmm_lognormal.json')))
    cfg['trainer'].update(save_dir=str(tmp_path), **trainer_over)
    cfg['data_loader']['args']['dims'] = [16, 16, 16]
    config = ConfigParser.from_dict(copy.deepcopy(cfg), timestamp='t')
    tm, rm = config.init_transformation_and_registration_modules()
    dl = config.init_data_loader()
    return Trainer(config, wrap(dl) if wrap else dl, config.init_losses(), tm, rm, config.init_metrics(), device=DEV)


KW = dict(no_chains=2, no_iters_burn_in=2, no_samples_MCMC=8, log_period_MCMC=4, save_outputs=False)
NAMES = ('MSE', 'NCC', 'MI', 'NMI')


def run_recorded(t, monkeypatch):
    """run t; -> (every metrics.update in order, the (step, moving image, rows) of every similarity call)"""
    updates, calls = [], []
    inner_update, inner_sim = t.metrics.update, t._image_similarity
    monkeypatch.setattr(t.metrics, 'update', lambda key, value, n=1: (updates.append((key, value)), inner_update(key, value, n))[1])

    def sim(fixed, moving_im):
        rows = inner_sim(fixed, moving_im)
        calls.append((fixed, moving_im.clone(), rows))
        return rows
    monkeypatch.setattr(t, '_image_similarity', sim)
    t.run()
    return updates, calls


def test_trainer_logs_the_similarity(tmp_path, monkeypatch):
    from ir_sgmcmc_amd.diagnostics import image_similarity_metric_names
    torch.manual_seed(0)
    on = make_trainer(tmp_path / 'on', image_similarity={'bins': 32, 'period': 3}, **KW)
    updates, calls = run_recorded(on, monkeypatch)
    C = on.no_chains
    res = on.metrics.result()
    new = image_similarity_metric_names(C)
    assert len(new) == 4 * (C + 2) and all(on.metrics._count[k] > 0 for k in new)
    # step 0, then logged steps 4 and 8 and the option's own period 3 after the burn-in of 2 (steps 5 and 8), then the mean
    assert [c[1].shape[0] for c in calls] == [1, C, C, C, 1]
    count = lambda key: sum(1 for k, _ in updates if k == key)
    assert count('VI/train/similarity/MI') == 1 and count('MCMC/chain_1/similarity/MI') == 3 and count('MCMC/similarity_of_mean/MI') == 1
    # the values logged last are those of the operator on the trainer's own images, last warped image and ranges
    fixed, warped, _ = calls[-2]
    want = calc_image_similarity(fixed['im'], warped, fixed['mask'][:1], 32, *on._similarity_ranges)
    for c in range(C):
        for k in NAMES:
            logged = [v for key, v in updates if key == f'MCMC/chain_{c}/similarity/{k}'][-1]
            assert logged == want[c][k.lower()] and math.isfinite(logged), (c, k)
        assert want[c]['n'] == int(fixed['mask'].sum()) and want[c]['n_clipped'] == 0 and want[c]['n_nonfinite'] == 0
        assert 0.0 < want[c]['ncc'] <= 1.0 and want[c]['mi'] > 0.0 and 1.0 < want[c]['nmi'] <= 2.0 and want[c]['mse'] > 0.0
    # the ranges are those of the pair
    from ir_sgmcmc_amd.data_loader import synthetic_pair
    f1, m1 = synthetic_pair((16, 16, 16))
    assert on._similarity_ranges == [(float(f1['im'].min()), float(f1['im'].max())), (float(m1['im'].min()), float(m1['im'].max()))]
    # the summary: the unregistered pair and the posterior-mean displacement, as logged
    s = on.similarity_summary
    assert set(s) == {'unregistered', 'mean'}
    for name, prefix in (('unregistered', 'VI/train/similarity'), ('mean', 'MCMC/similarity_of_mean')):
        assert s[name]['n'] == int(fixed['mask'].sum())
        for k in NAMES:
            assert s[name][k] == res[f'{prefix}/{k}'] and math.isfinite(s[name][k])
    unreg = calc_image_similarity(dev(f1['im'][None]), dev(m1['im'][None]), dev(f1['mask'][None]), 32, *on._similarity_ranges)[0]
    assert all(s['unregistered'][k] == unreg[k.lower()] for k in NAMES)
    assert s['mean']['MSE'] != s['unregistered']['MSE']
    # with the option off: the same chain, and exactly the keys of a run that has never heard of the option
    runs = {}
    for name, extra in (('off', {'image_similarity': False}), ('absent', {})):
        torch.manual_seed(0)
        runs[name] = make_trainer(tmp_path / name, **KW, **extra)
        runs[name].run()
    off, absent = runs['off'], runs['absent']
    bits = lambda x: x.view(torch.int32)
    assert torch.equal(bits(off.v_curr_state), bits(on.v_curr_state)) and torch.equal(bits(absent.v_curr_state), bits(on.v_curr_state))
    off_keys = list(off.metrics.result())
    assert off_keys == list(absent.metrics.result()) and [k for k in res if 'similarity' not in k] == off_keys
    assert sorted(res) == sorted(off_keys + new)
    assert off.similarity_options is None and off.similarity_summary is None and off._similarity_ranges is None


def test_trainer_logs_the_similarity_of_a_pair_without_segmentations(tmp_path):
    t = make_trainer(tmp_path, wrap=WithoutSegmentations, image_similarity=True, **KW)
    t.run()
    res = t.metrics.result()
    assert not any('/DSC/' in k and t.metrics._count[k] for k in res)
    for prefix in ['VI/train/similarity', 'MCMC/similarity_of_mean'] + [f'MCMC/chain_{c}/similarity' for c in range(t.no_chains)]:
        for k in NAMES:
            assert t.metrics._count[f'{prefix}/{k}'] > 0 and math.isfinite(res[f'{prefix}/{k}']), (prefix, k)
    assert t.similarity_options == {'bins': 64, 'period': None} and set(t.similarity_summary) == {'unregistered', 'mean'}
