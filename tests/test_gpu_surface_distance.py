"""ASD of label contours on the GPU (ops.label_surface_distance, calc_metrics, the trainer's ASD metrics) against a CPU
reference kept in this file: contours from shifted comparisons, distances by chunked brute force.  Exact by construction,
no code shared with the HIP path."""
import copy
import json
import math
import os

import numpy as np
import pytest
import torch

from ir_sgmcmc_amd import ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTURES = {'left_thalamus': 10, 'left_caudate': 11, 'left_putamen': 12, 'left_pallidum': 13, 'brain_stem': 16,
              'left_hippocampus': 17, 'left_amygdala': 18, 'left_accumbens': 26, 'right_thalamus': 49, 'right_caudate': 50,
              'right_putamen': 51, 'right_pallidum': 52, 'right_hippocampus': 53, 'right_amygdala': 54, 'right_accumbens': 58}
LABELS = list(STRUCTURES.values())
SPACING = (0.7, 1.3, 2.1)  # x (last axis), y, z


def ref_contour(mask):
    """voxels of `mask` with a face neighbour inside the volume that is not in `mask`"""
    out = np.zeros_like(mask)
    for ax in range(3):
        for sh in (1, -1):
            nb = np.roll(mask, sh, axis=ax)
            valid = np.ones_like(mask)
            edge = [slice(None)] * 3
            edge[ax] = 0 if sh == 1 else -1
            valid[tuple(edge)] = False
            out |= mask & valid & ~nb
    return out


def ref_directed_mean(a, b, s_zyx):
    pa = np.argwhere(a).astype(np.float64) * s_zyx
    pb = np.argwhere(b).astype(np.float64) * s_zyx
    total = 0.0
    step = max(1, 4_000_000 // len(pb))
    for i in range(0, len(pa), step):
        d2 = ((pa[i:i + step, None, :] - pb[None, :, :]) ** 2).sum(-1)
        total += np.sqrt(d2.min(axis=1)).sum()
    return total / len(pa)


def ref_asd(seg_fixed, seg_moving, labels, spacing):
    """(C, L) float64; seg_* numpy (Cf|C, 1, D, H, W)"""
    s_zyx = np.array([spacing[2], spacing[1], spacing[0]], dtype=np.float64)
    C = seg_moving.shape[0]
    out = np.zeros((C, len(labels)))
    for c in range(C):
        f = seg_fixed[c if seg_fixed.shape[0] > 1 else 0, 0]
        m = seg_moving[c, 0]
        for j, lab in enumerate(labels):
            a, b = ref_contour(f == lab), ref_contour(m == lab)
            if not a.any() or not b.any():
                out[c, j] = np.inf
            else:
                out[c, j] = 0.5 * (ref_directed_mean(a, b, s_zyx) + ref_directed_mean(b, a, s_zyx))
    return out


def gpu_asd(seg_fixed, seg_moving, labels=LABELS, spacing=SPACING):
    return ops.label_surface_distance(torch.from_numpy(seg_fixed).to(DEV), torch.from_numpy(seg_moving).to(DEV), labels,
                                      spacing).cpu().numpy()


def assert_same(got, want):
    assert got.shape == want.shape
    assert np.array_equal(np.isinf(got), np.isinf(want)), (got, want)
    fin = np.isfinite(want)
    np.testing.assert_allclose(got[fin], want[fin], rtol=1e-5)


# ------------------------------------------------------------------------------------------------ known answers
def test_single_voxels_give_the_scaled_distance():
    dims = (9, 12, 15)
    f = np.zeros((1, 1) + dims, np.int16)
    m = np.zeros((1, 1) + dims, np.int16)
    p, q = (1, 2, 3), (7, 10, 4)
    f[(0, 0) + p] = 10
    m[(0, 0) + q] = 10
    got = gpu_asd(f, m, [10, 11])
    d = math.sqrt(((p[2] - q[2]) * SPACING[0]) ** 2 + ((p[1] - q[1]) * SPACING[1]) ** 2 + ((p[0] - q[0]) * SPACING[2]) ** 2)
    assert got[0, 0] == pytest.approx(d, rel=1e-6)
    assert np.isinf(got[0, 1])


def test_half_spaces_at_256_cubed():
    """z < 128 against z < 131: the contours are the planes z = 127 and z = 130 (the volume border is not contour)"""
    N = 256
    f = torch.zeros(1, 1, N, N, N, dtype=torch.int16, device=DEV)
    m = torch.zeros(2, 1, N, N, N, dtype=torch.int16, device=DEV)
    f[:, :, :128] = 16
    m[:, :, :131] = 16
    got = ops.label_surface_distance(f, m, [16], SPACING).cpu().numpy()
    np.testing.assert_allclose(got, 3 * SPACING[2], rtol=1e-6)


# ------------------------------------------------------------------------------------------------ fuzz
def random_seg(rng, dims, labels, touch_border=True):
    D, H, W = dims
    seg = np.zeros(dims, np.int16)
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing='ij')
    for lab in labels:
        for _ in range(rng.integers(1, 3)):
            c = rng.uniform(0, 1, 3) * np.array(dims)
            r = rng.uniform(1.0, 0.25 * min(dims), 3)
            blob = ((z - c[0]) / r[0]) ** 2 + ((y - c[1]) / r[1]) ** 2 + ((x - c[2]) / r[2]) ** 2 < 1.0
            blob &= rng.uniform(size=dims) < 0.995  # holes make inner contours
            seg[blob] = lab
    if touch_border:
        seg[:, 0, :3] = labels[0]
    return seg


def fuzz_case(rng, dims, C, Cf):
    present = [l for l in LABELS if rng.uniform() < 0.8]
    f = np.stack([random_seg(rng, dims, present)[None] for _ in range(Cf)])
    m = np.stack([random_seg(rng, dims, [l for l in present if rng.uniform() < 0.9])[None] for _ in range(C)])
    # a single voxel, and a label whose box is the whole volume
    m[0, 0, dims[0] // 2, dims[1] // 2, dims[2] // 2] = 26
    f[0, 0, dims[0] // 3, dims[1] // 3, dims[2] // 3] = 26
    for s in (f, m):
        s[:, 0, 0, 0, 0] = 58
        s[:, 0, -1, -1, -1] = 58
        s[:, 0, dims[0] // 2:, :2, :] = 58
    return f, m


@pytest.mark.parametrize('dims', [(23, 37, 50), (64, 48, 80), (70, 66, 40), (9, 11, 150)])
@pytest.mark.parametrize('C,Cf', [(1, 1), (2, 1), (2, 2), (3, 3)])
def test_fuzz_against_cpu_reference(dims, C, Cf):
    rng = np.random.default_rng(hash((dims, C, Cf)) % 2**32)
    f, m = fuzz_case(rng, dims, C, Cf)
    assert_same(gpu_asd(f, m), ref_asd(f, m, LABELS, SPACING))


def test_realistic_ellipsoids_warped_by_a_displaced_chain():
    from ir_sgmcmc_amd.utils import RegistrationModule
    N, C = 128, 2
    rng = np.random.default_rng(7)
    z, y, x = np.meshgrid(*(np.arange(N),) * 3, indexing='ij')
    seg = np.zeros((N,) * 3, np.int16)
    for lab in LABELS:
        c = rng.uniform(0.25, 0.75, 3) * N
        r = rng.uniform(4, 14, 3)
        seg[((z - c[0]) / r[0]) ** 2 + ((y - c[1]) / r[1]) ** 2 + ((x - c[2]) / r[2]) ** 2 < 1.0] = lab
    g = torch.Generator().manual_seed(3)
    v = torch.nn.functional.interpolate(torch.randn(C, 3, 8, 8, 8, generator=g), size=(N,) * 3, mode='trilinear',
                                        align_corners=True) * 4.0
    transformation, _, _ = ops.svf_exp_fwd(v.to(DEV).contiguous())
    fixed = torch.from_numpy(seg)[None, None].to(DEV)
    warped = RegistrationModule()(fixed, transformation)
    assert not torch.equal(warped[0], fixed[0]) and not torch.equal(warped[0], warped[1])
    got = ops.label_surface_distance(fixed, warped, LABELS, SPACING).cpu().numpy()
    assert_same(got, ref_asd(fixed.cpu().numpy(), warped.cpu().numpy(), LABELS, SPACING))
    assert np.isfinite(got).all()


def test_two_calls_are_bit_identical():
    rng = np.random.default_rng(11)
    f, m = fuzz_case(rng, (70, 66, 40), 3, 1)
    fd, md = torch.from_numpy(f).to(DEV), torch.from_numpy(m).to(DEV)
    a = ops.label_surface_distance(fd, md, LABELS, SPACING)
    b = ops.label_surface_distance(fd, md, LABELS, SPACING)
    assert torch.equal(torch.nan_to_num(a, posinf=-1.0), torch.nan_to_num(b, posinf=-1.0))


def test_bad_arguments_are_refused():
    from ir_sgmcmc_amd import _lib as L
    seg = torch.zeros(2, 1, 8, 8, 8, dtype=torch.int16, device=DEV)
    with pytest.raises(L.IrsError):
        ops.label_surface_distance(seg[:1], seg, list(range(65)), SPACING)  # more than IRS_MAX_LABELS
    with pytest.raises(L.IrsError):
        ops.label_surface_distance(seg[:1], seg, [10], (1.0, 0.0, 1.0))
    with pytest.raises(L.IrsError):
        ops.label_surface_distance(torch.zeros(3, 1, 8, 8, 8, dtype=torch.int16, device=DEV), seg, [10], SPACING)
    with pytest.raises(L.IrsError):
        ops.label_surface_distance(seg.float(), seg, [10], SPACING)


# ------------------------------------------------------------------------------------------------ trainer
def make_trainer(tmp_path, **trainer_over):
    from ir_sgmcmc_amd.parse_config import ConfigParser
    from ir_sgmcmc_amd.trainer import Trainer
    cfg = json.load(open(os.path.join(ROOT, 'configs', 'synthetic_gmm_lognormal.json')))
    cfg['trainer'].update(save_dir=str(tmp_path), **trainer_over)
    cfg['data_loader']['args']['dims'] = [24, 24, 24]
    config = ConfigParser.from_dict(copy.deepcopy(cfg), timestamp='t')
    tm, rm = config.init_transformation_and_registration_modules()
    return Trainer(config, config.init_data_loader(), config.init_losses(), tm, rm, config.init_metrics(), device=DEV)


def test_trainer_logs_asd_of_every_chain(tmp_path):
    t = make_trainer(tmp_path, no_iters_burn_in=2, no_samples_MCMC=4, log_period_MCMC=2)
    t.run()
    res = t.metrics.result()
    for i in range(t.no_chains):
        for s in ('left_thalamus', 'brain_stem'):
            assert np.isfinite(res[f'MCMC/chain_{i}/ASD/{s}']) and res[f'MCMC/chain_{i}/ASD/{s}'] >= 0.0
        assert np.isinf(res[f'MCMC/chain_{i}/ASD/left_caudate'])
    # step 0: the unregistered pair
    assert np.isfinite(res['VI/train/ASD/left_thalamus']) and 'VI/train/DSC/brain_stem' in res


def test_vi_run_logs_asd(tmp_path):
    t = make_trainer(tmp_path, VI=True, no_iters_VI=2, no_samples_VI_test=1, log_period_VI=1, MCMC=False)
    t.run()
    res = t.metrics.result()
    for mode in ('train', 'test'):
        assert np.isfinite(res[f'VI/{mode}/ASD/left_thalamus']) and np.isinf(res[f'VI/{mode}/ASD/left_caudate'])


def test_calc_metrics_dice_is_calc_DSC_GPU():
    from ir_sgmcmc_amd.utils import calc_DSC_GPU, calc_metrics
    rng = np.random.default_rng(5)
    f, m = fuzz_case(rng, (23, 37, 50), 2, 1)
    fd, md = torch.from_numpy(f).to(DEV), torch.from_numpy(m).to(DEV)
    ASD, DSC = calc_metrics(fd, md, STRUCTURES, torch.tensor(SPACING), no_samples=2)
    assert ASD.shape == DSC.shape == (2, len(STRUCTURES)) and ASD.dtype == np.float64
    want = calc_DSC_GPU(2, fd.expand_as(md), md, STRUCTURES)
    assert np.array_equal(DSC, want, equal_nan=True)
    assert_same(ASD, ref_asd(f, m, LABELS, SPACING))
    # the trainer's fixed seg may be .expand()-ed over the chains
    ASD2, DSC2 = calc_metrics(fd.expand_as(md), md, STRUCTURES, SPACING, no_samples=2)
    assert np.array_equal(ASD2, ASD) and np.array_equal(DSC2, DSC, equal_nan=True)
