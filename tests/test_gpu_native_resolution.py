"""Native-resolution outputs on the device: ops.native_warp bit for bit on the exact cases (a zero field, integer translations
on the dyadic geometry, the border rule of the padded axis -- tests/test_native_resolution_host.py proves the expected volumes
exact), against the fp64 restatement of tests/_native_resolution.py on smooth fields within 4x the restatement's own fp32 band,
the millimetres of the native surface distances, and the trainer option."""
import copy
import functools
import json
import os

import numpy as np
import pytest
import torch

from ir_sgmcmc_amd import ops as G
from ir_sgmcmc_amd.native import NativeGrid
from ir_sgmcmc_amd.parse_config import ConfigParser
from ir_sgmcmc_amd.trainer import Trainer
from ir_sgmcmc_amd.utils import calc_native_metrics, transform_coordinates
from ir_sgmcmc_amd.utils.imageio import read_nifti, read_vtk_vectors
from tests import _native_resolution as R
from tests._report import check
from tests._native_resolution import write_pair

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(t):
    return t.to(DEV).contiguous()


def bits(t):
    return t.contiguous().view(torch.int32)


def first_mismatch(a, b):
    idx = (a != b).nonzero()
    return f'{idx.shape[0]} elements differ, first at {idx[0].tolist()}: {a[tuple(idx[0])].item()!r} != {b[tuple(idx[0])].item()!r}'


def run(u, grid, im, seg, mask, fill, scale):
    out = G.native_warp(dev(u), grid, im=dev(im), seg=dev(seg), mask=dev(mask), fill=fill, want_displacement=scale)
    return {k: v.cpu() for k, v in out.items()}


# ---------------------------------------------------------------- 1. exact, bit for bit
@pytest.mark.parametrize('shape, dims', [((10, 13, 16), (8, 8, 8)), ((6, 7, 5), (16, 16, 16))])
@pytest.mark.parametrize('C, Cim', [(1, 1), (2, 1), (2, 2)])
def test_zero_field_returns_the_moving_volumes(shape, dims, C, Cim):
    grid = NativeGrid.from_shape(shape, dims)
    im, seg, mask = R.random_volumes(shape, 6, Cim)
    got = run(torch.zeros(C, 3, *dims), grid, im, seg, mask, float(im.min()), grid.voxel_scale())
    for key, vol in (('im', im), ('seg', seg), ('mask', mask)):
        assert got[key].dtype == vol.dtype and got[key].shape == (C, 1, *shape)
        want = vol.expand(C, -1, -1, -1, -1)
        assert torch.equal(got[key], want), f'{key}: {first_mismatch(got[key], want)}'
    assert got['displacement'].shape == (C, 3, *shape) and not got['displacement'].any()


DYADIC = NativeGrid.from_shape((9, 17, 17), (9, 9, 9))   # p = (4, 0, 0), P = 17^3, grid step 0.5


@pytest.mark.parametrize('per_channel, shift', [
    ((2 * 2 / 16, 0.0, -2 * 1 / 16), (-1, 0, 2)),   # +2 voxels along the last axis, -1 along the first
    # 2. the border rule of the padded axis: +6 along the first axis (p0 = 4) reads the fill in the pad and beyond it
    ((0.0, 0.0, 2 * 6 / 16), (6, 0, 0)),
    ((2 * 20 / 16, 0.0, 0.0), (0, 0, 20)),          # along the unpadded last axis the last native column repeats
])
def test_integer_translations_bit_for_bit(per_channel, shift):
    im, seg, mask = R.random_volumes(DYADIC.shape, 5)
    fill = float(im.min())
    got = run(R.constant_field(2, DYADIC.dims, per_channel), DYADIC, im, seg, mask, fill, DYADIC.voxel_scale())
    for key, vol, f in (('im', im, fill), ('seg', seg, 0), ('mask', mask, False)):
        want = R.shifted(vol, DYADIC, shift, f).expand(2, -1, -1, -1, -1)
        assert torch.equal(got[key], want), f'{key}: {first_mismatch(got[key], want)}'
    for c in range(3):   # the displacement in native voxels; channel c belongs to axis 2 - c
        assert bool((got['displacement'][:, c] == shift[2 - c]).all())
    if shift == (6, 0, 0):
        assert bool((got['im'][:, 0, 3:] == fill).all()) and not got['seg'][:, 0, 3:].any()
    if shift == (0, 0, 20):
        assert torch.equal(got['im'][0, 0], im[0, 0, :, :, -1:].expand(-1, -1, 17))


def test_requested_outputs_only_and_the_same_bits():
    """every subset of the outputs comes from its own instantiation of the kernel: each gives what the full launch gives"""
    grid = NativeGrid.from_shape((11, 20, 14), (12, 10, 8), (2.0, 1.5, 1.0))
    u, (im, seg, mask) = dev(R.smooth_field(2, grid.dims, 3)), [dev(t) for t in R.random_volumes(grid.shape, 4)]
    full = G.native_warp(u, grid, im=im, seg=seg, mask=mask, fill=0.0, want_displacement=grid.mm_scale())
    assert sorted(full) == ['displacement', 'im', 'mask', 'seg']
    for keys in (('im',), ('seg',), ('mask',), ('displacement',), ('im', 'seg'), ('seg', 'mask'), ('im', 'displacement')):
        part = G.native_warp(u, grid, im=im if 'im' in keys else None, seg=seg if 'seg' in keys else None,
                             mask=mask if 'mask' in keys else None, fill=0.0,
                             want_displacement=grid.mm_scale() if 'displacement' in keys else None)
        assert sorted(part) == sorted(keys)
        for k in keys:
            assert torch.equal(part[k], full[k]), k
    assert float(full['im'].min()) >= 0.0   # fill = 0 <= the image: nothing below it
    default_fill = G.native_warp(u, grid, im=im)['im']   # the default fill is the image's minimum
    assert torch.equal(default_fill, G.native_warp(u, grid, im=im, fill=float(im.min()))['im'])


# ---------------------------------------------------------------- 3. against the float64 restatement
@functools.lru_cache(maxsize=None)
def smooth_case(shape, dims, C, bump):
    grid = NativeGrid.from_shape(shape, dims, (2.0, 1.5, 1.0))
    u = R.smooth_field(C, dims, 7)
    u[:, 1] += bump   # a constant added to one channel: sources leave the padded box
    im, seg, mask = R.random_volumes(shape, 3)   # Cim = 1: the chains share the moving volumes
    fill = float(im.min())
    ref = {dt: R.native_warp(u, grid, dt, im, seg, mask, fill, grid.mm_scale()) for dt in (torch.float32, torch.float64)}
    return grid, u, im, seg, mask, fill, ref, R.away_from_half(u, grid)


@pytest.mark.parametrize('shape, dims, C, bump', [
    ((10, 13, 16), (8, 8, 8), 1, 0.0),
    ((11, 20, 14), (12, 10, 8), 1, 0.0),
    ((33, 40, 37), (16, 16, 16), 2, 0.0),     # several blocks, a ragged tail on every axis, two chains sharing one volume
    ((11, 20, 14), (12, 10, 8), 1, 0.5),
])
def test_smooth_fields_against_the_float64_restatement(shape, dims, C, bump):
    """The HIP result may be at most 4x as far from the fp64 restatement as the restatement's own fp32 evaluation is (the
    factor covers a different, equally valid evaluation order in the fused kernel), floored at 1e-6 max|.|.  Measured on the
    MI355X: image errors 0.50, 0.78, 0.68 and 0.99 of the band at the four cases, displacement errors 1.00 of it at all four."""
    grid, u, im, seg, mask, fill, ref, keep = smooth_case(shape, dims, C, bump)
    r32, r64 = ref[torch.float32], ref[torch.float64]
    got = run(u, grid, im, seg, mask, fill, grid.mm_scale())
    T = f'native_warp/smooth {shape}->{dims} C={C} bump={bump}'
    vox = (r64['displacement'].abs() / torch.tensor(grid.zooms[::-1], dtype=torch.float64).view(1, 3, 1, 1, 1)).amax().item()
    print(f'\n{T}: largest displacement {vox:.2f} native voxels')
    assert 0.5 < vox < 8.0
    for key in ('im', 'displacement'):
        band = float((r32[key].double() - r64[key]).abs().max())
        bound = max(4.0 * band, 1e-6 * float(r64[key].abs().max()))
        err = float((got[key].double() - r64[key]).abs().max())
        print(f'{T}: {key}: fp32 band {band:.3e}, HIP error {err:.3e}, ratio {err / band:.2f}, bound {bound:.3e}')
        check(T, key, got[key], r64[key], bound)
    left_out = 1.0 - float(keep.float().mean())
    print(f'{T}: nearest: {100 * left_out:.3f} % of the voxels within 1e-3 of a half-integer source coordinate')
    assert left_out < 0.02
    for key in ('seg', 'mask'):
        wrong = (got[key] != r64[key]) & keep
        assert not wrong.any(), f'{key}: {first_mismatch(got[key].where(keep, r64[key]), r64[key])}'
        assert float((got[key] != r64[key]).float().mean()) <= left_out
    if bump:   # sources did leave the padded box along axis 1, where the border rule repeats the padded border: the fill
        q = R.source_coordinate(u, grid)
        assert float(q[:, 1].max()) > grid.padded[1] - 1 + 1.0


# ---------------------------------------------------------------- 4. millimetres
def test_native_surface_distances_are_in_mm_of_the_right_axis():
    shape, dims = (16, 14, 12), (8, 8, 8)
    a = torch.zeros(1, 1, *shape, dtype=torch.int16)
    b = torch.zeros_like(a)
    a[0, 0, 4:10, 4:10, 3:9] = 1
    b[0, 0, 6:12, 4:10, 3:9] = 1   # the same box two voxels further along axis 0
    u = torch.zeros(1, 3, *dims, device=DEV)
    hd, asd = {}, {}
    for zooms in ((2.0, 1.5, 1.0), (3.0, 1.5, 1.0), (1.0, 1.5, 2.0)):
        grid = NativeGrid.from_shape(shape, dims, zooms)
        m = calc_native_metrics(u, grid, dev(a), dev(b), {'box': 1}, percentiles=(95,))
        assert torch.equal(m['seg'].cpu(), b) and m['DSC'].shape == m['ASD'].shape == m['HD'].shape == (1, 1)
        hd[zooms], asd[zooms] = float(m['HD'][0, 0]), float(m['ASD'][0, 0])
        # the ASD is the one of the surface operator under the spacing written out by hand: sx is the zoom of the LAST axis
        by_hand = G.label_surface_distance(dev(a), dev(b), [1], (zooms[2], zooms[1], zooms[0]))
        assert float(by_hand[0, 0]) == asd[zooms]
        assert float(calc_native_metrics(u, grid, dev(a), dev(b), {'box': 1})['ASD'][0, 0]) == asd[zooms]
    # two voxels along axis 0 are 2 zooms[0] mm -- not 2 zooms[2]
    assert hd[(2.0, 1.5, 1.0)] == 4.0 and hd[(3.0, 1.5, 1.0)] == 6.0 and hd[(1.0, 1.5, 2.0)] == 2.0
    assert asd[(3.0, 1.5, 1.0)] > asd[(2.0, 1.5, 1.0)] > asd[(1.0, 1.5, 2.0)] > 0.0


# ---------------------------------------------------------------- 5. trainer
NATIVE, ZOOMS, N = (20, 26, 22), (1.0, 1.5, 2.0), 16


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


def test_trainer_native_resolution(tmp_path, monkeypatch):
    data_dir = write_pair(tmp_path / 'data', NATIVE, ZOOMS)
    kw = dict(no_chains=2, no_iters_burn_in=2, no_samples_MCMC=8, log_period_MCMC=4, save_samples=True, hausdorff=True)
    torch.manual_seed(0)
    a = make_trainer(tmp_path / 'a', data_dir, native_resolution={'period': 3, 'save': ['im', 'seg', 'displacement']}, **kw)
    seen = {}   # sample_no -> (the displacement of that step in voxels of the registration grid, whether it was saved)
    inner = a._log_native
    monkeypatch.setattr(a, '_log_native', lambda no, d, save: (seen.__setitem__(no, (d.clone(), save)), inner(no, d, save))[1])
    a.run()
    C, grid = a.no_chains, NativeGrid.from_shape(NATIVE, (N, N, N), ZOOMS)
    # logged steps 4 and 8 (saved), the option's own period 3 after the burn-in of 2: steps 5 and 8
    assert sorted(seen) == [4, 5, 8] and [seen[k][1] for k in (4, 5, 8)] == [True, False, True]
    res = a.metrics.result()
    names = ['DSC', 'ASD', 'HD', 'HD95']
    keys = [f'MCMC/chain_{c}/native/{k}/{s}' for c in range(C) for k in names for s in a.structures_dict]
    assert a.structures_dict and all(k in res for k in keys)
    present = [s for s, label in a.structures_dict.items() if label in (10, 16, 49)]   # the labels of the synthetic pair
    assert len(present) == 3
    for c in range(C):
        for s in present:
            assert 0.0 < res[f'MCMC/chain_{c}/native/DSC/{s}'] <= 1.0
            assert 0.0 <= res[f'MCMC/chain_{c}/native/ASD/{s}'] <= res[f'MCMC/chain_{c}/native/HD/{s}'] < float('inf')
    pair = a.data_loader.native()
    seg_moving, im_moving = dev(pair['moving']['seg'].unsqueeze(0)), dev(pair['moving']['im'].unsqueeze(0))
    folder = a.config.save_dirs['samples'] / 'MCMC'
    for no in (4, 8):
        want = G.native_warp(transform_coordinates(seen[no][0]).contiguous(), grid, im=im_moving, seg=seg_moving,
                             fill=pair['fill']['moving'], want_displacement=grid.mm_scale())
        for c in range(C):
            stem = f'chain_{c}_sample_{no:07}'
            seg, zooms = read_nifti(str(folder / f'{stem}_seg_moving_warped_native.nii.gz'), np.int16)
            assert seg.shape == NATIVE and zooms == ZOOMS and (seg == want['seg'][c, 0].cpu().numpy()).all()
            im, zooms = read_nifti(str(folder / f'{stem}_im_moving_warped_native.nii.gz'))
            assert im.shape == NATIVE and zooms == ZOOMS and (im == want['im'][c, 0].cpu().numpy()).all()
            kind, dims, field = read_vtk_vectors(str(folder / f'{stem}_displacement_native.vtk'))
            assert dims == NATIVE and (field == want['displacement'][c].cpu().numpy()).all()
    assert not list(folder.glob('chain_*_sample_0000005_*native*'))
    # the posterior mean on the native grid
    top = a.config.save_dirs['samples']
    mean = G.native_warp(transform_coordinates(a.displacement_mean.unsqueeze(0)).contiguous(), grid, im=im_moving,
                         fill=pair['fill']['moving'], want_displacement=grid.mm_scale())
    kind, dims, field = read_vtk_vectors(str(top / 'MCMC_sample_mean_native.vtk'))
    assert dims == NATIVE and (field == mean['displacement'][0].cpu().numpy()).all() and float(abs(field).max()) > 0
    im, zooms = read_nifti(str(top / 'MCMC_im_moving_warped_mean_native.nii.gz'))
    assert im.shape == NATIVE and zooms == ZOOMS and (im == mean['im'][0, 0].cpu().numpy()).all()
    # with the option off or absent: the same chain bit for bit, no native key, no native file
    runs = {}
    for name, extra in (('off', {'native_resolution': False}), ('absent', {})):
        torch.manual_seed(0)
        runs[name] = make_trainer(tmp_path / name, data_dir, **kw, **extra)
        runs[name].run()
    off, absent = runs['off'], runs['absent']
    assert torch.equal(bits(off.v_curr_state), bits(a.v_curr_state)) and torch.equal(bits(absent.v_curr_state), bits(a.v_curr_state))
    assert torch.equal(bits(off.displacement_mean), bits(a.displacement_mean)) and torch.equal(bits(off.displacement_std), bits(a.displacement_std))
    off_keys = list(off.metrics.result())
    assert off_keys == list(absent.metrics.result()) and [k for k in res if '/native/' not in k] == off_keys
    assert all(res[k] == off.metrics.result()[k] or res[k] != res[k] for k in off_keys)
    for t in (off, absent):
        assert t.native_options is None and t._native is None
    files = lambda tr: sorted(str(p.relative_to(tr.config.save_dirs['samples'])) for p in tr.config.save_dirs['samples'].rglob('*') if p.is_file())
    assert files(off) == files(absent) == [f for f in files(a) if 'native' not in f] and len(files(a)) == len(files(off)) + 2 * C * 3 + 2
    # a loader without native volumes is refused with a message that says so
    cfg = json.load(open(os.path.join(ROOT, 'configs', 'synthetic_gmm_lognormal.json')))
    cfg['trainer'].update(save_dir=str(tmp_path / 'syn'), native_resolution=True)
    cfg['data_loader']['args']['dims'] = [N, N, N]
    config = ConfigParser.from_dict(cfg, timestamp='t')
    tm, rm = config.init_transformation_and_registration_modules()
    with pytest.raises(ValueError, match='has no native volumes'):
        Trainer(config, config.init_data_loader(), config.init_losses(), tm, rm, config.init_metrics(), device=DEV)
