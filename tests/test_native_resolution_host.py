"""Host side of the native-resolution outputs: the geometry class against what BiobankDataset does, the zooms through
`native_pair()`, the `trainer.native_resolution` option, the refusals of the data set, the loaders and the C ABI (none of
which reaches a launch), and the proof that the exact cases of the GPU test are exact: on an integer translation the fp32 and
the fp64 evaluation of tests/_native_resolution.py both equal the shifted volume, fill and border included."""
import ctypes as C

import numpy as np
import pytest
import torch

from ir_sgmcmc_amd import _lib as L
from ir_sgmcmc_amd import ops
from ir_sgmcmc_amd.data_loader.data_loaders import BiobankDataLoader, SyntheticDataLoader
from ir_sgmcmc_amd.data_loader.datasets import BiobankDataset
from ir_sgmcmc_amd.data_loader.synthetic import synthetic_pair
from ir_sgmcmc_amd.diagnostics import native_resolution_options
from ir_sgmcmc_amd.native import NativeGrid
from tests import _native_resolution as R
from tests._native_resolution import write_pair

ZOOMS = (1.0, 1.5, 2.0)


# ---------------------------------------------------------------- geometry
@pytest.mark.parametrize('shape, dims, padding, padded', [
    ((9, 17, 17), (9, 9, 9), (4, 0, 0), (17, 17, 17)),
    ((10, 13, 16), (8, 8, 8), (3, 1, 0), (16, 15, 16)),     # odd padding: the padded volume is not a cube
    ((6, 7, 5), (16, 16, 16), (0, 0, 1), (6, 7, 7)),        # the grid finer than the image
])
def test_native_grid_numbers(shape, dims, padding, padded, tmp_path):
    g = NativeGrid.from_shape(shape, dims, ZOOMS)
    assert (g.shape, g.padding, g.padded, g.dims, g.zooms) == (shape, padding, padded, dims, ZOOMS)
    first, last = g.grid_coordinate((0, 0, 0)), g.grid_coordinate(tuple(n - 1 for n in shape))
    for a in range(3):
        assert first[a] == padding[a] * (dims[a] - 1) / (padded[a] - 1) >= 0.0
        assert last[a] == (shape[a] - 1 + padding[a]) * (dims[a] - 1) / (padded[a] - 1) <= dims[a] - 1
    # channel 0 belongs to the last axis
    assert g.voxel_scale() == ((padded[2] - 1) / 2, (padded[1] - 1) / 2, (padded[0] - 1) / 2)
    assert g.mm_scale() == ((padded[2] - 1) / 2 * 2.0, (padded[1] - 1) / 2 * 1.5, (padded[0] - 1) / 2 * 1.0)
    # the padding is the data set's for the same file
    ds = BiobankDataset(dims, write_pair(tmp_path / 'data', shape))
    ds[0]
    assert ds.padding == tuple((p, p) for p in padding)
    assert ds.native_pair()['grid'] == g


def test_dyadic_case_sits_on_the_half_voxel_lattice():
    g = NativeGrid.from_shape((9, 17, 17), (9, 9, 9))
    assert g.grid_coordinate((0, 0, 0)) == (2.0, 0.0, 0.0) and g.grid_coordinate((1, 1, 1)) == (2.5, 0.5, 0.5)
    assert g.voxel_scale() == (8.0, 8.0, 8.0) and g.zooms == (1.0, 1.0, 1.0)


def test_spacing_xyz_is_last_axis_first():
    g = NativeGrid.from_shape((4, 5, 6), (4, 4, 4), (2.0, 1.5, 1.0))
    assert g.spacing_xyz() == (1.0, 1.5, 2.0)   # sx scales the LAST axis of the array, whose zoom is zooms[2]
    assert g.zooms == (2.0, 1.5, 1.0)


@pytest.mark.parametrize('shape, dims, zooms', [((4, 5), (4, 4, 4), ZOOMS), ((0, 5, 6), (4, 4, 4), ZOOMS), ((4, 5, 6), (4, 1, 4), ZOOMS),
                                                ((4, 5, 6), (4, 4, 4), (1.0, 0.0, 1.0)), ((4, 5, 6), (4, 4, 4), (1.0, float('nan'), 1.0)),
                                                ((1, 1, 1), (4, 4, 4), ZOOMS)])
def test_native_grid_refusals(shape, dims, zooms):
    with pytest.raises(ValueError):
        NativeGrid.from_shape(shape, dims, zooms)


# ---------------------------------------------------------------- data set and loaders
def test_native_pair_keeps_the_volumes_and_the_header_zooms(tmp_path):
    shape, dims = (10, 13, 16), (8, 8, 8)
    root = write_pair(tmp_path / 'data', shape)
    dl = BiobankDataLoader(data_dir=root, dims=dims)
    (fixed, moving, vp), = list(dl)
    # what the loader yielded before is what it yields now
    assert sorted(fixed) == sorted(moving) == ['im', 'mask', 'seg'] and sorted(vp) == ['log_var', 'mu', 'u']
    assert tuple(fixed['im'].shape) == (1, 1, *dims) and fixed['mask'].dtype == torch.bool and fixed['seg'].dtype == torch.int16
    assert torch.equal(dl.im_spacing, torch.tensor(16 / np.asarray(dims), dtype=torch.float32))
    assert dl.dataset.zooms == ZOOMS
    pair = dl.native()
    assert pair['grid'] == NativeGrid.from_shape(shape, dims, ZOOMS)
    want = synthetic_pair(shape, seed=3)
    for side, vol in zip(('fixed', 'moving'), want):
        got = pair[side]
        assert torch.equal(got['im'], vol['im']) and got['im'].dtype == torch.float32
        assert torch.equal(got['mask'], vol['mask']) and got['mask'].dtype == torch.bool
        assert torch.equal(got['seg'], vol['seg']) and got['seg'].dtype == torch.int16
        assert pair['fill'][side] == float(vol['im'].min())


def test_mismatched_shapes_are_refused(tmp_path):
    root = write_pair(tmp_path / 'data', (10, 13, 16), moving_shape=(10, 13, 15))
    with pytest.raises(ValueError, match=r'shape \(10, 13, 15\) differs from \(10, 13, 16\).*one shape'):
        BiobankDataLoader(data_dir=root, dims=(8, 8, 8)).native()


def test_loaders_without_native_volumes():
    assert SyntheticDataLoader((8, 8, 8)).native is None
    assert BiobankDataLoader(data_dir=None, dims=(8, 8, 8), allow_synthetic_fallback=True).native is None


# ---------------------------------------------------------------- the option
def cfg(**over):
    return {'no_samples_MCMC': 8, 'log_period_MCMC': 4, 'no_chains': 2, **over}


def test_options_off_and_defaults():
    for off in ({}, {'native_resolution': False}, {'native_resolution': None}):
        assert native_resolution_options(cfg(**off)) is None
        assert native_resolution_options(cfg(**off), SyntheticDataLoader((8, 8, 8))) is None   # off: any loader will do
    assert native_resolution_options(cfg(native_resolution=True)) == {'period': None, 'save': ('im',)}
    assert native_resolution_options(cfg(native_resolution={})) == {'period': None, 'save': ('im',)}
    got = native_resolution_options(cfg(native_resolution={'period': 2, 'save': ['displacement', 'im', 'seg']}))
    assert got == {'period': 2, 'save': ('im', 'seg', 'displacement')}
    assert native_resolution_options(cfg(native_resolution={'save': []}))['save'] == ()


@pytest.mark.parametrize('opt, message', [
    ({'periodd': 2}, r"trainer\.native_resolution: unknown keys \['periodd'\]; known: \['period', 'save'\]"),
    ({'period': 0}, r'trainer\.native_resolution: the period must be >= 1, got 0'),
    ({'period': -3}, r'trainer\.native_resolution: the period must be >= 1, got -3'),
    ({'period': 2.0}, r'trainer\.native_resolution\.period must be an integer, got 2\.0'),
    ({'period': True}, r'trainer\.native_resolution\.period must be an integer, got True'),
    ({'save': 'im'}, r"trainer\.native_resolution\.save must be a list of distinct names out of \['im', 'seg', 'displacement'\], got 'im'"),
    ({'save': ['im', 'mask']}, r"trainer\.native_resolution\.save must be a list of distinct names .* got \['im', 'mask'\]"),
    ({'save': ['im', 'im']}, r"trainer\.native_resolution\.save must be a list of distinct names .* got \['im', 'im'\]"),
    ('yes', r'trainer\.native_resolution must be true, false or \{"period": P, "save": \[\.\.\.\]\}, got \'yes\''),
    (1, r'trainer\.native_resolution must be true, false or '),
])
def test_options_refusals(opt, message):
    with pytest.raises(ValueError, match=message):
        native_resolution_options(cfg(native_resolution=opt))


def test_option_refuses_a_loader_without_native_volumes(tmp_path):
    with pytest.raises(ValueError, match=r'trainer\.native_resolution: the data loader \(SyntheticDataLoader\) has no native volumes'):
        native_resolution_options(cfg(native_resolution=True), SyntheticDataLoader((8, 8, 8)))
    dl = BiobankDataLoader(data_dir=write_pair(tmp_path / 'data', (6, 7, 5)), dims=(8, 8, 8))
    assert native_resolution_options(cfg(native_resolution=True), dl) == {'period': None, 'save': ('im',)}


# ---------------------------------------------------------------- the operator's refusals (before any launch: CPU-safe)
def test_cpu_tensors_are_refused():
    g = NativeGrid.from_shape((6, 7, 5), (4, 4, 4))
    with pytest.raises(L.IrsError, match='GPU only'):
        ops.native_warp(torch.zeros(1, 3, 4, 4, 4), g, im=torch.zeros(1, 1, 6, 7, 5))
    with pytest.raises(L.IrsError, match='registration grid'):
        ops.native_warp(torch.zeros(1, 3, 4, 4, 5), g, im=torch.zeros(1, 1, 6, 7, 5))
    with pytest.raises(L.IrsError, match='nothing asked for'):
        ops.native_warp(torch.zeros(1, 3, 4, 4, 4), g)
    with pytest.raises(L.IrsError, match='does not match the native grid'):
        ops.native_warp(torch.zeros(1, 3, 4, 4, 4), g, seg=torch.zeros(1, 1, 6, 7, 6, dtype=torch.int16))
    with pytest.raises(L.IrsError, match='seg must be torch.int16'):
        ops.native_warp(torch.zeros(1, 3, 4, 4, 4), g, seg=torch.zeros(1, 1, 6, 7, 5))


PTR = C.c_void_p(4096)   # stands for a device pointer: every call below is refused before anything is launched or read


def abi_call(C_=1, dims=(4, 4, 4), native=(6, 7, 5), padding=(0, 0, 1), im=PTR, Cim=1, fill=0.0, scale=(1.0, 1.0, 1.0),
             im_out=PTR, seg_out=None, disp_out=None):
    lib = L.load()
    i3 = lambda v: (C.c_int32 * 3)(*v)
    return lib.irs_native_warp(PTR, C_, i3(dims), i3(native), i3(padding), im, None, None, Cim, fill,
                               (C.c_float * 3)(*scale) if scale is not None else None, im_out, seg_out, None, disp_out, None)


@pytest.mark.parametrize('kw, message', [
    (dict(native=(0, 7, 5)), r'native\[0\] = 0 < 1'),
    (dict(padding=(0, -1, 1)), r'padding\[1\] = -1 < 0'),
    (dict(native=(1, 7, 5)), r'padded extent 1 of axis 0, >= 2 needed'),
    (dict(dims=(4, 4, 1)), r'dims\[2\] = 1 < 2'),
    (dict(disp_out=PTR, scale=(1.0, float('inf'), 1.0)), r'scale\[1\] = inf, a finite value needed'),
    (dict(disp_out=PTR, scale=(float('nan'), 1.0, 1.0)), r'scale\[0\] = nan, a finite value needed'),
    (dict(disp_out=PTR, scale=None), r'displacement_out needs scale'),
    (dict(im_out=None), r'no output requested'),
    (dict(C_=0), r'C = 0 chains, 1\.\.8'),
    (dict(C_=9), r'C = 9 chains, 1\.\.8'),
    (dict(C_=2, Cim=3), r'moving volumes of 3 chains, 1 or 2 needed'),
    (dict(seg_out=PTR), r'an output is requested of a moving volume that is NULL'),
    (dict(fill=float('nan')), r'fill = nan, a finite value needed'),
    (dict(native=(1024, 1024, 1024), padding=(0, 0, 0)), r'fewer than 2\^30 voxels'),
])
def test_abi_refusals(kw, message):
    import re
    assert abi_call(**kw) != 0
    assert re.search(message, L.load().irs_last_error().decode()), L.load().irs_last_error().decode()


# ---------------------------------------------------------------- the exact cases of the GPU test are exact
DYADIC = NativeGrid.from_shape((9, 17, 17), (9, 9, 9))


@pytest.mark.parametrize('per_channel, shift', [
    ((0.0, 0.0, 0.0), (0, 0, 0)),
    ((2 * 2 / 16, 0.0, -2 * 1 / 16), (-1, 0, 2)),   # +2 voxels along the last axis, -1 along the first
    ((0.0, 0.0, 2 * 6 / 16), (6, 0, 0)),            # past the pad of the first axis (p0 = 4)
    ((2 * 20 / 16, 0.0, 0.0), (0, 0, 20)),          # past the unpadded last axis: its last column repeats
])
def test_integer_translations_are_exact(per_channel, shift):
    im, seg, mask = R.random_volumes(DYADIC.shape, 5)
    fill = float(im.min())
    u = R.constant_field(2, DYADIC.dims, per_channel)
    want = {'im': R.shifted(im, DYADIC, shift, fill), 'seg': R.shifted(seg, DYADIC, shift, 0), 'mask': R.shifted(mask, DYADIC, shift, False)}
    for dtype in (torch.float32, torch.float64):
        got = R.native_warp(u, DYADIC, dtype, im, seg, mask, fill, DYADIC.voxel_scale())
        for key in want:
            assert got[key].shape == (2, 1, *DYADIC.shape)
            assert torch.equal(got[key][0].to(want[key].dtype), want[key][0]) and torch.equal(got[key][0], got[key][1]), (key, dtype)
        d = got['displacement']
        for c in range(3):   # the displacement in native voxels, channel c <-> axis 2 - c
            assert bool((d[:, c] == shift[2 - c]).all())
    if shift == (6, 0, 0):   # rows whose source falls in the pad or beyond it read the fill
        assert bool((want['im'][0, 0, 3:] == fill).all()) and not bool((want['im'][0, 0, :3] == fill).all())
        assert not want['seg'][0, 0, 3:].any()
    if shift == (0, 0, 20):
        assert torch.equal(want['im'][0, 0], im[0, 0, :, :, -1:].expand(-1, -1, 17))


def test_restatement_at_zero_field_returns_the_volumes():
    for shape, dims in (((10, 13, 16), (8, 8, 8)), ((6, 7, 5), (16, 16, 16))):
        g = NativeGrid.from_shape(shape, dims)
        im, seg, mask = R.random_volumes(shape, 6)
        got = R.native_warp(torch.zeros(1, 3, *dims), g, torch.float64, im, seg, mask)
        assert torch.equal(got['im'].float(), im) and torch.equal(got['seg'], seg) and torch.equal(got['mask'], mask)
