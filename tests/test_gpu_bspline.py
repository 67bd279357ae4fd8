"""Cubic B-spline output resampling on the GPU (include/irsgmcmc.h, "Cubic B-spline output resampling"): the prefilter and
irs_bspline_warp bit for bit against the numpy restatement of tests/_bspline.py, the sharpness claim against an analytic image,
irs_native_warp_cubic against the float64 restatement and irs_native_warp, every refusal of the three entry points, and the
trainer with `trainer.output_interpolation`.

Measured on the CPU with the restatement: the 24^3 blob image under a smooth displacement of up to 1.7
voxels comes back with an RMS error of 6.30e-3 trilinearly and 2.23e-3 through the spline (a ratio of 2.8); only the order is
asserted.  The native bands are in tests/golden/bspline_bands.json (tests/golden/make_bspline_bands.py).

The voxels the native test leaves out are those within 1e-3 of a face of the native box ON A PADDED AXIS: where p_a = 0 the box
face is the face of the padded box, the border clamp puts whole rows of positions exactly on it and decides their class the same
way in any precision (counting those rows as "near a face" would leave out 3 to 28 % of the voxels; without them it is 0.04 to
0.15 %, under the 2 % cap)."""
import copy
import ctypes as C
import functools
import gzip
import json
import os

import numpy as np
import pytest
import torch

from ir_sgmcmc_amd import _lib as L
from ir_sgmcmc_amd import bspline, ops as G
from ir_sgmcmc_amd.native import NativeGrid
from ir_sgmcmc_amd.ops import _call
from ir_sgmcmc_amd.parse_config import ConfigParser
from ir_sgmcmc_amd.trainer import Trainer
from ir_sgmcmc_amd.utils import transform_coordinates
from ir_sgmcmc_amd.utils.imageio import read_nifti
from tests import _affine as A
from tests import _bspline as B
from tests import _native_resolution as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = 70 * 2.0 ** -24  # times max|c|: 64 products and the weights

# (2,3,70): extent 2 and a ragged second tile; (9,9,130): three tiles along x, the last ragged; (70,3,5): long z lines and fewer
# than 64 x-lines
SHAPES = [(2, 3, 70), (5, 6, 7), (12, 13, 44), (9, 9, 130), (70, 3, 5)]
# 2 n - 2 <= 32 holds at n = 17 and not at 18, on every axis
SWITCH = [(18, 5, 6), (17, 5, 6), (5, 18, 6), (5, 17, 6), (5, 6, 18), (5, 6, 17)]


def dev(t):
    return (torch.tensor(t) if isinstance(t, np.ndarray) else t).to(DEV).contiguous()


def bits(t):
    t = torch.tensor(t) if isinstance(t, np.ndarray) else t.cpu().contiguous()
    return t.view(torch.int32)


def same_bits(got, want):
    g, w = bits(got), bits(want)
    if torch.equal(g, w):
        return True
    idx = (g != w).nonzero()
    a, b = got.cpu().numpy() if torch.is_tensor(got) else got, want.cpu().numpy() if torch.is_tensor(want) else want
    at = tuple(idx[0].tolist())
    print(f'{idx.shape[0]} of {g.numel()} elements differ, first at {at}: {a[at]!r} != {b[at]!r}')
    return False


@functools.lru_cache(maxsize=None)
def volumes(shape, Cim, seed=0):
    """(image (Cim,1,*shape) float32, its restated coefficients), numpy; computed once and never written to"""
    im = torch.rand(Cim, 1, *shape, generator=torch.Generator().manual_seed(seed + 7 * Cim)).numpy()
    coeff = B.prefilter(im)
    im.setflags(write=False)
    coeff.setflags(write=False)
    return im, coeff


# ---------------------------------------------------------------- prefilter
@pytest.mark.parametrize('Cim', [1, 2])
@pytest.mark.parametrize('shape', SHAPES + SWITCH)
def test_prefilter_bit_for_bit(shape, Cim):
    im, want = volumes(shape, Cim)
    x = dev(im.copy())
    got = bspline.prefilter(x)
    assert same_bits(got, want)
    assert same_bits(bspline.prefilter(x), got)  # two calls
    assert same_bits(x, im)  # the input was left alone
    _call('irs_bspline_prefilter', L.dev_ptr(x), L.dev_ptr(x), Cim, *shape)  # in place
    assert same_bits(x, want)


# ---------------------------------------------------------------- warp
def transformation(shape, C, kind):
    ident = R.identity(shape, torch.float32)
    if kind == 'identity':
        t = ident.expand(C, -1, -1, -1, -1)
    elif kind == 'smooth':
        t = ident + R.smooth_field(C, shape, seed=5, amp=0.5)
    else:  # leaves the box by two voxels on every side of every axis
        scale = torch.tensor([(n - 1 + 4.0) / (n - 1) for n in reversed(shape)]).view(1, 3, 1, 1, 1)
        t = (ident * scale + 0.1 * R.smooth_field(C, shape, seed=6, amp=0.5)).expand(C, -1, -1, -1, -1)
    return t.contiguous()


@pytest.mark.parametrize('kind', ['smooth', 'clamp', 'identity'])
@pytest.mark.parametrize('C, Cim', [(1, 1), (2, 1), (2, 2)])
@pytest.mark.parametrize('shape', SHAPES)
def test_warp_bit_for_bit(shape, C, Cim, kind):
    im, coeff = volumes(shape, Cim)
    t = transformation(shape, C, kind)
    if kind == 'clamp':  # the case does what it is for
        q = B.index_coordinates(t[0].numpy())
        assert all(qa.min() <= -1.5 and qa.max() >= n - 1 + 1.5 for qa, n in zip(q, shape))
    got = bspline.warp(dev(coeff), dev(t))
    assert got.shape == (C, 1, *shape) and same_bits(got, B.warp(coeff, t.numpy()))
    if kind == 'identity':
        err = float((got.cpu() - torch.tensor(im)).abs().max())
        assert err <= NODE * float(np.abs(coeff).max()), err


def test_sharper_than_trilinear():
    """the analytic blob image on 24^3 under a smooth displacement: both interpolants against the function itself at the
    warped positions -- the spline is closer"""
    dims = (24, 24, 24)
    f = A.blob_function(dims, seed=0)
    k = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in dims], indexing='ij'), -1)
    im = dev(f(k).astype(np.float32)[None, None])
    t = (R.identity(dims, torch.float32) + R.smooth_field(1, dims, 3)).contiguous()
    q = [np.clip(qa, 0, n - 1) for qa, n in zip(B.index_coordinates(t[0].numpy(), np.float64), dims)]
    truth = f(np.stack(q, -1))
    rms = lambda x: float(np.sqrt(np.mean((x[0, 0].cpu().numpy().astype(np.float64) - truth) ** 2)))
    linear, cubic = rms(G.warp(im, dev(t))), rms(bspline.warp(bspline.prefilter(im), dev(t)))
    print(f'RMS error against the analytic image: trilinear {linear:.4g}, cubic B-spline {cubic:.4g}, ratio {linear / cubic:.3g}')
    assert cubic < linear


# ---------------------------------------------------------------- native
BANDS = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'bspline_bands.json')))['cases']


@pytest.mark.parametrize('seed', B.NATIVE_SEEDS)
@pytest.mark.parametrize('shape, dims', B.NATIVE_CASES)
def test_native_cubic(shape, dims, seed):
    grid, u, im, fill = B.native_inputs(shape, dims, seed)
    coeff = torch.from_numpy(B.prefilter(im.numpy()))
    ref = B.native_float64(u, grid, im, coeff, fill)
    keep, cubic = ~ref['near_face'], ref['cubic']
    left_out, share = float(ref['near_face'].mean()), float((~cubic)[keep].mean())
    print(f'{shape} at {dims}, padding {grid.padding}: {left_out:.4f} left out, fall-back share {share:.4f}')
    assert left_out <= 0.02
    assert share == 0.0 if max(grid.padding) == 0 else 0.10 <= share <= 0.30
    got = bspline.native_warp_cubic(dev(u), grid, dev(im), dev(coeff), fill).cpu()[:, 0]
    linear = G.native_warp(dev(u), grid, im=dev(im), fill=fill)['im'].cpu()[:, 0]
    fall = torch.from_numpy(keep & ~cubic)
    assert torch.equal(bits(got)[fall], bits(linear)[fall])
    sel = keep & cubic
    err = float(np.abs(got.numpy().astype(np.float64) - ref['value'])[sel].max())
    band = BANDS['x'.join(map(str, shape))]['band']
    print(f'cubic voxels: max deviation from float64 {err:.3g}, band {band:.3g}')
    assert err <= band
    # the coefficients default to the prefilter of the image, the fill to its minimum
    assert torch.equal(bits(bspline.native_warp_cubic(dev(u), grid, dev(im)).cpu()[:, 0]), bits(got))


@pytest.mark.parametrize('shape, dims', B.NATIVE_CASES)
def test_native_cubic_zero_displacement(shape, dims):
    grid, u, im, fill = B.native_inputs(shape, dims, 1)
    coeff = torch.from_numpy(B.prefilter(im.numpy()))
    got = bspline.native_warp_cubic(dev(torch.zeros_like(u)), grid, dev(im), dev(coeff), fill).cpu()
    assert float((got - im).abs().max()) <= NODE * float(coeff.abs().max())


# ---------------------------------------------------------------- refusals: nothing is launched, P is no device pointer
P = 0x1000
MAXC = L.IRS_MAX_CHAINS
NAN, INF = float('nan'), float('inf')
DIMS = dict(D=4, H=4, W=4)


def i32(*v):
    return (C.c_int32 * len(v))(*v)


GOOD = {
    'irs_bspline_prefilter': dict(im=P, coeff=P, Cim=2, **DIMS, stream=None),
    'irs_bspline_warp': dict(coeff=P, Cim=1, transformation=P, out=P, C=2, **DIMS, stream=None),
    'irs_native_warp_cubic': dict(displacement=P, C=2, dims=i32(4, 4, 4), native=i32(6, 6, 6), padding=i32(1, 1, 1), im=P, coeff=P,
                                  Cim=1, fill=0.0, im_out=P, stream=None),
}
CASES = []


def case(cid, fn, expected, **bad):
    assert bad and set(bad) <= set(GOOD[fn]), (cid, fn)
    CASES.append((f'{fn[4:]}-{cid}', fn, bad, f'{fn}: {expected}'))


PF, BW, NC = 'irs_bspline_prefilter', 'irs_bspline_warp', 'irs_native_warp_cubic'
for fn, args in ((PF, ['im', 'coeff']), (BW, ['coeff', 'transformation', 'out']),
                 (NC, ['displacement', 'dims', 'native', 'padding', 'im', 'coeff', 'im_out'])):
    for arg in args:
        case(f'{arg}=null', fn, 'null pointer', **{arg: None})
for fn in (PF, BW):
    for axis in 'DHW':
        dims = {**DIMS, axis: 1}
        case(f'{axis}=1', fn, f'dims ({dims["D"]}, {dims["H"]}, {dims["W"]}), every one >= 2 needed', **{axis: 1})
    case('voxels=2^30', fn, 'the volume must have fewer than 2^30 voxels', D=1024, H=1024, W=1024)
    case('grid-planes', fn, 'dims (32768, 4, 4) x 2 volumes exceed the launch grid', D=32768)
    case('grid-rows', fn, 'dims (4, 262141, 4) x 2 volumes exceed the launch grid', H=262141)
case('Cim=0', PF, f'Cim = 0 volumes, 1..{MAXC}', Cim=0)
case('Cim=max+1', PF, f'Cim = {MAXC + 1} volumes, 1..{MAXC}', Cim=MAXC + 1)
for fn in (BW, NC):
    case('C=0', fn, f'C = 0 chains, 1..{MAXC}', C=0)
    case('C=max+1', fn, f'C = {MAXC + 1} chains, 1..{MAXC}', C=MAXC + 1)
for n in (0, 3):
    case(f'Cim={n}', BW, f'coefficients of {n} chains, 1 or 2 needed', Cim=n)
    case(f'Cim={n}', NC, f'moving volumes of {n} chains, 1 or 2 needed', Cim=n)
case('native=1', NC, 'native[1] = 1 < 2', native=i32(6, 1, 6))
case('padding=-1', NC, 'padding[2] = -1 < 0', padding=i32(1, 1, -1))
case('dims=1', NC, 'dims[2] = 1 < 2', dims=i32(4, 4, 1))
case('extent=2^24', NC, 'padded extent 16777216 of axis 1 is not exact in float32', native=i32(6, 1 << 24, 6), padding=i32(1, 0, 1))
case('voxels=2^30', NC, 'the native volume must have fewer than 2^30 voxels', native=i32(1024, 1024, 1024))
case('dims=2^30', NC, 'bad dims', dims=i32(1024, 1024, 1024))
case('grid-planes', NC, 'native shape (32768, 6, 6) x 2 chains exceeds the launch grid', native=i32(32768, 6, 6))
case('grid-rows', NC, 'native shape (6, 262141, 6) x 2 chains exceeds the launch grid', native=i32(6, 262141, 6))
for what, v, shown in (('nan', NAN, 'nan'), ('inf', INF, 'inf'), ('-inf', -INF, '-inf')):
    case(f'fill={what}', NC, f'fill = {shown}, a finite value needed', fill=v)


@pytest.mark.parametrize('fn,bad,expected', [pytest.param(*c[1:], id=c[0]) for c in CASES])
def test_refusal(fn, bad, expected):
    lib = L.load()
    rc = getattr(lib, fn)(*{**GOOD[fn], **bad}.values())
    got = lib.irs_last_error().decode()
    assert rc == 1 and got == expected, (rc, got)


def test_wrapper_refusals():
    im = torch.rand(1, 1, 4, 5, 6, device=DEV)
    with pytest.raises(L.IrsError, match='float32'):
        bspline.prefilter(im.double())
    with pytest.raises(L.IrsError, match='does not match'):
        bspline.warp(im, torch.zeros(1, 3, 4, 5, 7, device=DEV))
    grid = NativeGrid.from_shape((4, 5, 6), (8, 8, 8))
    with pytest.raises(L.IrsError, match='registration grid'):
        bspline.native_warp_cubic(torch.zeros(1, 3, 8, 8, 9, device=DEV), grid, im)
    with pytest.raises(L.IrsError, match='fill must be finite'):
        bspline.native_warp_cubic(torch.zeros(1, 3, 8, 8, 8, device=DEV), grid, im, fill=float('nan'))


# ---------------------------------------------------------------- trainer
N = 16
RUN = dict(no_chains=2, no_iters_burn_in=2, no_samples_MCMC=4, log_period_MCMC=2, save_samples=True)


def make_trainer(tmp_path, data_loader=None, **trainer_over):
    cfg = json.load(open(os.path.join(ROOT, 'configs', 'synthetic_gmm_lognormal.json')))
    cfg['trainer']['save_dir'] = str(tmp_path)
    cfg['data_loader']['args']['dims'] = [N, N, N]
    if data_loader is not None:
        cfg['data_loader'] = data_loader
    cfg['trainer'].update(trainer_over)
    config = ConfigParser.from_dict(copy.deepcopy(cfg), timestamp='t')
    dl = config.init_data_loader()
    losses = config.init_losses()
    tm, rm = config.init_transformation_and_registration_modules()
    return Trainer(config, dl, losses, tm, rm, config.init_metrics(), device=DEV)


def run(tmp_path, name, data_loader=None, spy=None, **over):
    torch.manual_seed(0)
    t = make_trainer(tmp_path / name, data_loader, **over)
    if spy is not None:
        spy(t)
    t.run()
    return t


def files(t):
    """everything the run wrote but its log, its copy of the configuration and its checkpoints: relative path -> content"""
    top = t.config.save_dirs['dir']
    # (a .gz file is compared unpacked: its gzip header holds the second it was written in)
    content = lambda p: gzip.decompress(p.read_bytes()) if p.suffix == '.gz' else p.read_bytes()
    return {str(p.relative_to(top)): content(p) for key in ('tensors', 'samples', 'images', 'fields', 'grids', 'norms')
            for p in sorted(t.config.save_dirs[key].rglob('*')) if p.is_file()}


def spy_saved_image(monkeypatch, seen):
    """-> a hook for run(): every call of Trainer._saved_image leaves (the trilinear image, the transformation) in `seen`"""
    def spy(t):
        inner = t._saved_image

        def wrapped(warped, transformation):
            seen.append((warped.clone(), transformation.clone()))
            return inner(warped, transformation)
        monkeypatch.setattr(t, '_saved_image', wrapped)
    return spy


def same_metrics(a, b):
    ra, rb = a.metrics.result(), b.metrics.result()
    return list(ra) == list(rb) and all(ra[k] == rb[k] or (ra[k] != ra[k] and rb[k] != rb[k]) for k in ra)


def test_trainer_output_interpolation(tmp_path, monkeypatch):
    seen = []
    cubic = run(tmp_path, 'cubic', spy=spy_saved_image(monkeypatch, seen), **RUN, output_interpolation='cubic')
    again = run(tmp_path, 'again', **RUN, output_interpolation='cubic')
    absent = run(tmp_path, 'absent', **RUN)
    linear = run(tmp_path, 'linear', **RUN, output_interpolation='linear')
    assert cubic.interpolation_options == {'order': 3} and absent.interpolation_options is None and absent._spline_coeff is None
    fc, fa = files(cubic), files(absent)
    assert fc == files(again)                 # two runs are bit-identical
    assert fa == files(linear)                # "linear" is the key absent
    assert list(fc) == list(fa)               # no file more, no file less
    changed = sorted(k for k in fc if fc[k] != fa[k])
    warped = sorted(k for k in fc if 'im_moving_warped' in k)
    assert changed == warped and len(warped) == 2 * 2, (changed, warped)  # samples 4 and 6 of two chains
    assert same_metrics(cubic, absent) and same_metrics(cubic, again) and same_metrics(linear, absent)
    assert torch.equal(bits(cubic.v_curr_state), bits(absent.v_curr_state))
    assert torch.equal(bits(cubic.displacement_mean), bits(absent.displacement_mean))
    # the saved image is bspline.warp of the saved transformation, and not the trilinear image
    assert len(seen) == 2
    folder = cubic.config.save_dirs['samples'] / 'MCMC'
    for (trilinear, t), no in zip(seen, (4, 6)):
        want = bspline.warp(cubic._spline_coeff, t.contiguous()).cpu().numpy()
        for c in range(2):
            im, _ = read_nifti(str(folder / f'chain_{c}_sample_{no:07}_im_moving_warped.nii.gz'))
            assert im.dtype == np.float32 and (im == want[c, 0]).all() and (im != trilinear[c, 0].cpu().numpy()).any()
    with pytest.raises(ValueError, match='"linear" or "cubic"'):
        make_trainer(tmp_path / 'bad', **RUN, output_interpolation='quintic')


def test_trainer_vi_output_interpolation(tmp_path, monkeypatch):
    """the saved VI test sample and im_moving_warped_mu: the spline at the transformation the stage formed"""
    seen = []
    t = run(tmp_path, 'vi', spy=spy_saved_image(monkeypatch, seen), VI=True, MCMC=False, no_iters_VI=2, no_samples_VI_test=1,
            log_period_VI=1, output_interpolation='cubic')
    assert len(seen) == 2
    dirs = t.config.save_dirs
    for (trilinear, tr), path in zip(seen, (dirs['samples'] / 'VI' / 'sample_0000001_im_moving_warped.nii.gz',
                                            dirs['images'] / 'im_moving_warped_mu.nii.gz')):
        im, _ = read_nifti(str(path))
        want = bspline.warp(t._spline_coeff, tr.contiguous())[0, 0].cpu().numpy()
        assert (im == want).all() and (im != trilinear[0, 0].cpu().numpy()).any()


NATIVE, ZOOMS = (20, 26, 22), (1.0, 1.5, 2.0)


def test_trainer_native_output_interpolation(tmp_path, monkeypatch):
    data_dir = R.write_pair(tmp_path / 'data', NATIVE, ZOOMS)
    loader = {'type': 'BiobankDataLoader', 'args': {'data_dir': data_dir, 'dims': [N, N, N], 'sigma_v_init': 0.5, 'u_v_init': 0.1}}
    kw = dict(no_chains=2, no_iters_burn_in=2, no_samples_MCMC=4, log_period_MCMC=4, save_samples=True,
              native_resolution={'save': ['im', 'seg']})
    seen = {}

    def spy(t):
        inner = t._log_native
        monkeypatch.setattr(t, '_log_native', lambda no, d, save: (seen.__setitem__(no, d.clone()), inner(no, d, save))[1])

    cubic = run(tmp_path, 'cubic', loader, spy, **kw, output_interpolation='cubic')
    absent = run(tmp_path, 'absent', loader, **kw)
    fc, fa = files(cubic), files(absent)
    changed = sorted(k for k in fc if fc[k] != fa[k])
    warped = sorted(k for k in fc if 'im_moving_warped' in k)
    # per chain the sample image and its native twin, and the native image of the posterior mean
    assert list(fc) == list(fa) and changed == warped and len(warped) == 2 * 2 + 1, (changed, warped)
    assert same_metrics(cubic, absent)
    pair = cubic.data_loader.native()
    grid = NativeGrid.from_shape(NATIVE, (N, N, N), ZOOMS)
    im_moving = dev(pair['moving']['im'].unsqueeze(0))
    coeff = bspline.prefilter(im_moving)
    assert torch.equal(bits(coeff), bits(cubic._native['coeff']))
    assert sorted(seen) == [4]
    want = bspline.native_warp_cubic(transform_coordinates(seen[4]).contiguous(), grid, im_moving, coeff, pair['fill']['moving'])
    folder = cubic.config.save_dirs['samples']
    for c in range(2):
        im, zooms = read_nifti(str(folder / 'MCMC' / f'chain_{c}_sample_0000004_im_moving_warped_native.nii.gz'))
        assert im.shape == NATIVE and zooms == ZOOMS and (im == want[c, 0].cpu().numpy()).all()
    mean = bspline.native_warp_cubic(transform_coordinates(cubic.displacement_mean.unsqueeze(0)).contiguous(), grid, im_moving, coeff,
                                     pair['fill']['moving'])
    im, _ = read_nifti(str(folder / 'MCMC_im_moving_warped_mean_native.nii.gz'))
    assert (im == mean[0, 0].cpu().numpy()).all()
