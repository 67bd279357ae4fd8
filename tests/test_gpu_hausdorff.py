"""Hausdorff and percentile surface distances on the GPU (ops.label_hausdorff_distance, calc_surface_metrics, the trainer's
`hausdorff` option) against the CPU restatement of tests/_hausdorff.py, which shares no code with the HIP path.

Bitwise where the transform is exact: with unit spacing every squared distance is an integer, and an isotropic power-of-two
spacing scales numerator and denominator of the envelope intersections alike, so the GPU must return exactly
sqrt(float64(float32(d2))).  With the anisotropic spacing the float32 transform rounds: rtol 1e-5, as the ASD test."""
import copy
import json
import math
import os

import numpy as np
import pytest
import torch

from ir_sgmcmc_amd import _lib as L
from ir_sgmcmc_amd import ops
from tests import _hausdorff as HD

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABELS = HD.LABELS
SPACING = (0.7, 1.3, 2.1)  # x (last axis), y, z
PCTS = (1.0, 50.0, 95.0, 100.0)
DIMS = [(23, 37, 50), (64, 48, 80), (70, 66, 40), (9, 11, 150)]
CHAINS = [(1, 1), (2, 1), (3, 3)]


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # a copy: the shared fuzz maps are read-only


def gpu_hd(f, m, labels=LABELS, spacing=SPACING, percentiles=(95,)):
    out = ops.label_hausdorff_distance(dev(f), dev(m), labels, spacing, percentiles)
    return {k: v.cpu().numpy() for k, v in out.items()}


def check_shapes(out, C, n_labels, Q):
    assert out['asd'].shape == out['hd'].shape == (C, n_labels) and out['hd_directed'].shape == (C, n_labels, 2)
    assert out['hd_pct'].shape == (Q, C, n_labels) and out['hd_pct_directed'].shape == (Q, C, n_labels, 2)
    for v in out.values():
        assert v.dtype == np.float64 and not np.isnan(v).any()
    assert np.array_equal(out['hd'], out['hd_directed'].max(-1)) and np.array_equal(out['hd_pct'], out['hd_pct_directed'].max(-1))


def expected(d2, scale=1.0):
    """what the device reports for the exact squared distance d2 * scale"""
    return np.sqrt((d2 * scale).astype(np.float32).astype(np.float64))


# ------------------------------------------------------------------------------------------------ known answers
def test_single_voxels_give_the_scaled_distance_in_every_output():
    """fixes the axis mapping; each directed set holds one voxel"""
    dims = (9, 12, 15)
    f = np.zeros((1, 1) + dims, np.int16)
    m = np.zeros((1, 1) + dims, np.int16)
    p, q = (1, 2, 3), (7, 10, 4)
    f[(0, 0) + p] = 10
    m[(0, 0) + q] = 10
    out = gpu_hd(f, m, [10, 11], percentiles=(1e-6, 50, 95, 100))
    check_shapes(out, 1, 2, 4)
    d = math.sqrt(((p[2] - q[2]) * SPACING[0]) ** 2 + ((p[1] - q[1]) * SPACING[1]) ** 2 + ((p[0] - q[0]) * SPACING[2]) ** 2)
    for k, v in out.items():
        np.testing.assert_allclose(v[..., 0, :] if k.endswith('directed') else v[..., 0], d, rtol=1e-6, err_msg=k)
        assert np.isinf(v[..., 1, :] if k.endswith('directed') else v[..., 1]).all(), k  # the absent label


def half_spaces(za, zb):
    f = np.zeros((1, 1, 24, 20, 70), np.int16)
    m = np.zeros((1, 1, 24, 20, 70), np.int16)
    f[:, :, :za] = 16
    m[:, :, :zb] = 16
    return f, m


def test_half_spaces_all_ties():
    """z < 10 against z < 13: the contours are the planes z = 9 and z = 12, every distance is 3 sz"""
    out = gpu_hd(*half_spaces(10, 13), [16], percentiles=PCTS)
    check_shapes(out, 1, 1, 4)
    for k, v in out.items():
        np.testing.assert_allclose(v, 3 * SPACING[2], rtol=1e-6, err_msg=k)


def test_one_stray_voxel_moves_the_maximum_only():
    """the same slab in both maps, and one voxel of the label 10 planes above its face in the moving one"""
    f, m = half_spaces(10, 10)
    m[0, 0, 19, 7, 33] = 16
    out = gpu_hd(f, m, [16], percentiles=(95,))
    np.testing.assert_allclose(out['hd_directed'][0, 0], [0.0, 10 * SPACING[2]], rtol=1e-6)
    assert np.array_equal(out['hd_pct_directed'][0, 0, 0], [0.0, 0.0])
    assert out['hd'][0, 0] > out['hd_pct'][0, 0, 0] == 0.0


def test_absent_label_gives_inf_everywhere():
    f, m = HD.fuzz_maps((23, 37, 50), 2, 1)
    out = gpu_hd(f, m, [99, 10], percentiles=(50, 95))
    check_shapes(out, 2, 2, 2)
    for k, v in out.items():
        assert np.isposinf(v[..., 0, :] if k.endswith('directed') else v[..., 0]).all(), k


# ------------------------------------------------------------------------------------------------ fuzz
def assert_matches(out, ref, scale, exact):
    want_hd, want_pct = expected(ref['hd2'], scale), expected(ref['pct2'], scale)
    for got, want, name in ((out['hd_directed'], want_hd, 'hd'), (out['hd_pct_directed'], want_pct, 'hd_pct')):
        assert got.shape == want.shape, name
        assert np.array_equal(np.isinf(got), np.isinf(want)), name
        if exact:
            bad = got != want
            assert not bad.any(), (name, int(bad.sum()), got[bad][:4], want[bad][:4])
        else:
            fin = np.isfinite(want)
            np.testing.assert_allclose(got[fin], want[fin], rtol=1e-5, err_msg=name)
    assert np.array_equal(np.isinf(out['asd']), np.isinf(ref['asd']))


@pytest.mark.parametrize('dims', DIMS)
@pytest.mark.parametrize('C,Cf', CHAINS)
def test_fuzz_bitwise_with_dyadic_isotropic_spacing(dims, C, Cf):
    f, m = HD.fuzz_maps(dims, C, Cf)
    ref = HD.fuzz_reference(dims, C, Cf, (1.0, 1.0, 1.0), PCTS)
    assert np.isfinite(ref['hd2']).sum() >= 8 and (ref['pct2'][2] < ref['hd2'])[np.isfinite(ref['hd2'])].any()
    for s in (1.0, 0.5):
        out = gpu_hd(f, m, spacing=(s, s, s), percentiles=PCTS)
        check_shapes(out, C, len(LABELS), 4)
        assert_matches(out, ref, s * s, exact=True)
        fin = np.isfinite(ref['asd'])
        np.testing.assert_allclose(out['asd'][fin], s * ref['asd'][fin], rtol=1e-6)


@pytest.mark.parametrize('dims', DIMS)
@pytest.mark.parametrize('C,Cf', CHAINS)
def test_fuzz_with_anisotropic_spacing(dims, C, Cf):
    f, m = HD.fuzz_maps(dims, C, Cf)
    ref = HD.fuzz_reference(dims, C, Cf, SPACING, PCTS)
    out = gpu_hd(f, m, percentiles=PCTS)
    assert_matches(out, ref, 1.0, exact=False)
    fin = np.isfinite(ref['asd'])
    np.testing.assert_allclose(out['asd'][fin], ref['asd'][fin], rtol=1e-5)


def test_whole_volume_box_with_lines_longer_than_the_lds_envelope():
    """label 58 of the fuzz maps touches two opposite corners: its box is the 70 x 66 x 40 volume, 70 planes deep, so pass D
    keeps its envelopes in global scratch"""
    dims, j = (70, 66, 40), LABELS.index(58)
    f, m = HD.fuzz_maps(dims, 2, 1)
    for s in (f, m):
        zyx = np.argwhere(s[0, 0] == 58)
        assert (zyx.min(0) == 0).all() and (zyx.max(0) == np.array(dims) - 1).all()
    ref = HD.fuzz_reference(dims, 2, 1, (1.0, 1.0, 1.0), PCTS)
    out = gpu_hd(f, m, [58], spacing=(1.0, 1.0, 1.0), percentiles=PCTS)
    assert np.isfinite(out['hd']).all()
    assert_matches(out, {k: v[..., j:j + 1, :] if k != 'asd' else v[:, j:j + 1] for k, v in ref.items()}, 1.0, exact=True)


# ------------------------------------------------------------------------------------------------ invariants
@pytest.mark.parametrize('spacing', [(1.0, 1.0, 1.0), SPACING])
def test_invariants(spacing):
    f, m = HD.fuzz_maps((70, 66, 40), 3, 3)
    fd, md = dev(f), dev(m)
    a = ops.label_hausdorff_distance(fd, md, LABELS, spacing, PCTS)
    b = ops.label_hausdorff_distance(fd, md, LABELS, spacing, PCTS)
    for k in a:  # two calls are bit-identical
        assert torch.equal(a[k], b[k]), k
    assert torch.isfinite(a['hd']).sum() >= 8
    # the selection at q = 100 and the maximum of pass D are independent code paths
    assert torch.equal(a['hd_pct_directed'][-1], a['hd_directed']) and torch.equal(a['hd_pct'][-1], a['hd'])
    assert (a['hd_pct_directed'][1:] >= a['hd_pct_directed'][:-1]).all()  # inf >= inf holds
    assert torch.equal(a['asd'], ops.label_surface_distance(fd, md, LABELS, spacing))
    # fewer percentiles select the same values
    c = ops.label_hausdorff_distance(fd, md, LABELS, spacing, (95.0,))
    assert torch.equal(c['hd_pct_directed'][0], a['hd_pct_directed'][2]) and torch.equal(c['hd_directed'], a['hd_directed'])


# ------------------------------------------------------------------------------------------------ edge cases
def test_smallest_rank_and_no_percentiles():
    dims = (23, 37, 50)
    f, m = HD.fuzz_maps(dims, 1, 1)
    ref = HD.fuzz_reference(dims, 1, 1, (1.0, 1.0, 1.0), (1e-9, 100.0))  # k = 0: the smallest distance
    out = gpu_hd(f, m, spacing=(1.0, 1.0, 1.0), percentiles=(1e-9, 100.0))
    assert_matches(out, ref, 1.0, exact=True)
    none = gpu_hd(f, m, spacing=(1.0, 1.0, 1.0), percentiles=())
    check_shapes(none, 1, len(LABELS), 0)
    assert np.array_equal(none['hd_directed'], out['hd_directed']) and np.array_equal(none['asd'], out['asd'])


def test_64_labels():
    f, m = HD.fuzz_maps((23, 37, 50), 2, 1)
    many = LABELS + [l for l in range(100, 200) if l not in LABELS][:64 - len(LABELS)]
    assert len(many) == L.IRS_MAX_LABELS
    out, few = gpu_hd(f, m, many, percentiles=(50, 95)), gpu_hd(f, m, percentiles=(50, 95))
    check_shapes(out, 2, 64, 2)
    for k in out:
        sel = (Ellipsis, slice(0, len(LABELS)), slice(None)) if k.endswith('directed') else (Ellipsis, slice(0, len(LABELS)))
        rest = (Ellipsis, slice(len(LABELS), None), slice(None)) if k.endswith('directed') else (Ellipsis, slice(len(LABELS), None))
        assert np.array_equal(out[k][sel], few[k]) and np.isposinf(out[k][rest]).all(), k
    assert np.isfinite(few['hd']).any()


def test_bad_arguments_are_refused():
    seg = torch.zeros(2, 1, 8, 8, 8, dtype=torch.int16, device=DEV)
    bad = [dict(labels=list(range(65))), dict(spacing=(1.0, 0.0, 1.0)), dict(spacing=(1.0, float('inf'), 1.0)),
           dict(spacing=(1.0, 1.0)), dict(percentiles=(0.0,)), dict(percentiles=(100.5,)), dict(percentiles=(95.0, 95.0)),
           dict(percentiles=(99.0, 95.0)), dict(percentiles=(float('nan'),)), dict(percentiles=(10, 20, 30, 40, 50)),
           dict(fixed=torch.zeros(3, 1, 8, 8, 8, dtype=torch.int16, device=DEV)), dict(fixed=seg.float())]
    for kw in bad:
        args = dict(fixed=seg[:1], labels=[10], spacing=SPACING, percentiles=(95,))
        args.update(kw)
        with pytest.raises(L.IrsError):
            ops.label_hausdorff_distance(args['fixed'], seg, args['labels'], args['spacing'], args['percentiles'])
    out = ops.label_hausdorff_distance(seg[:1], seg, [10], SPACING)  # and the call still works afterwards
    assert torch.isinf(out['hd']).all() and out['hd_pct'].shape == (1, 2, 1)


def test_calc_surface_metrics():
    from ir_sgmcmc_amd.utils import calc_metrics, calc_surface_metrics
    f, m = HD.fuzz_maps((23, 37, 50), 2, 1)
    fd, md = dev(f), dev(m)
    sm = calc_surface_metrics(fd, md, HD.STRUCTURES, torch.tensor(SPACING), percentiles=(50, 95), no_samples=2)
    assert sm['ASD'].shape == sm['HD'].shape == (2, len(LABELS)) and sm['HDp'].shape == (2, 2, len(LABELS))
    assert all(v.dtype == np.float64 for v in sm.values())
    assert np.array_equal(sm['ASD'], calc_metrics(fd, md, HD.STRUCTURES, SPACING, no_samples=2)[0])
    out = gpu_hd(f, m, percentiles=(50, 95))
    assert np.array_equal(sm['HD'], out['hd']) and np.array_equal(sm['HDp'], out['hd_pct'])
    # the trainer's fixed map may be .expand()-ed over the chains; fewer samples than maps
    sm2 = calc_surface_metrics(fd.expand_as(md), md, HD.STRUCTURES, SPACING, percentiles=(50, 95), no_samples=2)
    assert all(np.array_equal(sm2[k], sm[k]) for k in sm)
    sm1 = calc_surface_metrics(fd, md, HD.STRUCTURES, SPACING, percentiles=(50, 95))
    assert np.array_equal(sm1['HD'], sm['HD'][:1]) and np.array_equal(sm1['HDp'], sm['HDp'][:, :1])


# ------------------------------------------------------------------------------------------------ trainer
SHIFT = 3


class MisalignedSegmentation:
    """The loader of the config with its moving segmentation moved SHIFT voxels along z.  The synthetic pair carries the same
    label map in both images, and the few transitions of a test warp it by less than a voxel: nearly every contour distance is
    then 0, so HD95 = 0 < ASD, correctly (a 95th percentile exceeds the mean only when more than 5 % of the contour has moved).
    Moved by 3 voxels, the unregistered pair has ASD 1.08, HD95 2.83 and HD 3 for both present structures (CPU restatement,
    checked below), which a warp of less than a voxel cannot bring under the ASD."""

    def __init__(self, loader):
        self.loader = loader

    def __getattr__(self, name):
        return getattr(self.loader, name)

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for fixed, moving, var_params in self.loader:
            moving = dict(moving, seg=torch.roll(moving['seg'], SHIFT, dims=2))  # (1, 1, D, H, W): dim 2 is z
            yield fixed, moving, var_params


def make_trainer(tmp_path, **trainer_over):
    from ir_sgmcmc_amd.parse_config import ConfigParser
    from ir_sgmcmc_amd.trainer import Trainer
    cfg = json.load(open(os.path.join(ROOT, 'configs', 'synthetic_gmm_lognormal.json')))
    cfg['trainer'].update(save_dir=str(tmp_path), **trainer_over)
    cfg['data_loader']['args']['dims'] = [24, 24, 24]
    config = ConfigParser.from_dict(copy.deepcopy(cfg), timestamp='t')
    tm, rm = config.init_transformation_and_registration_modules()
    return Trainer(config, MisalignedSegmentation(config.init_data_loader()), config.init_losses(), tm, rm, config.init_metrics(),
                   device=DEV)


def check_prefix(res, prefix, present=('left_thalamus', 'brain_stem')):
    for s in present:
        for k in ('HD', 'HD95'):
            assert np.isfinite(res[f'{prefix}/{k}/{s}']) and res[f'{prefix}/{k}/{s}'] >= res[f'{prefix}/ASD/{s}'], (prefix, k, s)
        assert res[f'{prefix}/HD/{s}'] >= res[f'{prefix}/HD95/{s}']
    for k in ('ASD', 'HD', 'HD95'):
        assert np.isposinf(res[f'{prefix}/{k}/left_caudate']), (prefix, k)


def test_trainer_logs_hd_next_to_every_asd(tmp_path):
    on = make_trainer(tmp_path / 'on', no_iters_burn_in=2, no_samples_MCMC=4, log_period_MCMC=2, hausdorff=True)
    on.run()
    res = on.metrics.result()
    for i in range(on.no_chains):
        check_prefix(res, f'MCMC/chain_{i}')
    check_prefix(res, 'VI/train')  # step 0: the unregistered pair
    # ... whose values are known: unit spacing, so bit for bit those of the CPU restatement
    from ir_sgmcmc_amd.data_loader import synthetic_pair
    seg = synthetic_pair((24, 24, 24))[0]['seg'].numpy()[None]
    labels = [HD.STRUCTURES[s] for s in ('left_thalamus', 'brain_stem')]
    ref = HD.reference(seg, np.roll(seg, SHIFT, axis=2), labels, (1.0, 1.0, 1.0), (95.0,))
    for j, s in enumerate(('left_thalamus', 'brain_stem')):
        assert res[f'VI/train/HD/{s}'] == expected(ref['hd2'][0, j]).max() == float(SHIFT)
        assert res[f'VI/train/HD95/{s}'] == expected(ref['pct2'][0, 0, j]).max() < float(SHIFT)
        assert res[f'VI/train/ASD/{s}'] == pytest.approx(ref['asd'][0, j], rel=1e-6)
    off = make_trainer(tmp_path / 'off', no_iters_burn_in=2, no_samples_MCMC=4, log_period_MCMC=2)
    off.run()
    res_off = off.metrics.result()
    assert not any('/HD' in k for k in res_off)
    assert set(res_off) == {k for k in res if '/HD' not in k}
    # the ASD of the combined call is the ASD of the separate one
    assert res_off['VI/train/ASD/left_thalamus'] == res['VI/train/ASD/left_thalamus']


def test_vi_run_logs_hd(tmp_path):
    t = make_trainer(tmp_path, VI=True, no_iters_VI=2, no_samples_VI_test=1, log_period_VI=1, MCMC=False,
                     hausdorff={'percentiles': [95, 99]})
    t.run()
    res = t.metrics.result()
    for mode in ('train', 'test'):
        check_prefix(res, f'VI/{mode}', present=('left_thalamus',))  # the structure the ASD test of the VI stage relies on
        for s in ('left_thalamus', 'brain_stem'):
            assert res[f'VI/{mode}/HD/{s}'] >= res[f'VI/{mode}/HD99/{s}'] >= res[f'VI/{mode}/HD95/{s}'] >= 0.0
