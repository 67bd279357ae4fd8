"""The surface posterior on the device (ops.surface_posterior_update / _finalize, diagnostics.SurfacePosterior,
utils.calc_surface_posterior, the trainer option) against the float64 numpy restatement of tests/_surface_posterior.py, whose
docstring derives the tolerances: with the dyadic spacings used here every squared distance is exact in float32, the samples
agree with the restatement to the one rounding of the root, and only the float32 recurrence contributes beyond that.

Every contour voxel is compared, the counts for equality everywhere, and the state off the contours for equality with what it
held before the first update.  The largest fraction of a bound used is recorded through tests/_report.check and stated in
DESIGN.md section 6."""
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
from ir_sgmcmc_amd.diagnostics import SurfacePosterior, recorded_steps, surface_metric_names
from tests import _surface_posterior as SP
from tests._report import check

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = (0.5, 0.9, 0.95)
ANISO = (0.5, 1.0, 2.0)  # x (last axis), y, z


def dev(a):
    return torch.from_numpy(np.array(a, order='C')).to(DEV)  # a contiguous copy: the shared case maps are read-only


def fresh_state(dims, off=None):
    """zero state; with `off` (a bool map) the voxels there hold sentinels no update may touch"""
    mean, m2, count = np.zeros(dims, np.float32), np.zeros(dims, np.float32), np.zeros(dims, np.int32)
    if off is not None:
        mean[off], m2[off], count[off] = 7.5, -2.25, -3
    return dev(mean), dev(m2), dev(count)


def run(fixed, moving, labels, spacing, state=None):
    """fixed (D,H,W), moving (steps, C, D, H, W) -> the state after the steps, as numpy"""
    f = dev(fixed)[None, None]
    state = state or fresh_state(fixed.shape)
    for step in moving:
        ops.surface_posterior_update(f, dev(step)[:, None], labels, spacing, *state)
    return state


def finalize(fixed, labels, state, levels=LEVELS, mask=None):
    out = ops.surface_posterior_finalize(dev(fixed)[None, None], labels, *state, levels, None if mask is None else dev(mask))
    return [t.cpu().numpy() for t in out]


# ------------------------------------------------------------------------------------------------ known answers
@pytest.mark.parametrize('spacing', [(1.0, 1.0, 1.0), ANISO])
def test_known_answers(spacing):
    """single voxels, half-spaces for a < b and a > b, identical maps: the sample at every contour voxel as defined, and with equal
    records the final mean equals the sample bit for bit and m2 == 0"""
    p, q = (1, 2, 3), (4, 0, 5)
    cases = [(SP.single_voxels((6, 5, 7), p, q), [10, 11], np.float32(SP.point_distance(p, q, spacing)))]
    for a, b in ((4, 7), (7, 4)):
        cases.append((SP.half_spaces((3, 4, 12), a, b), [16], np.float32((a - b) * spacing[0])))
    f5 = SP.case_maps((5, 7, 9), 1)[0]
    cases.append(((f5, f5[None]), SP.LABELS3, np.float32(0.0)))
    for (f, m), labels, want in cases:
        on = SP.fixed_contours(f, labels) >= 0
        assert on.any()
        for steps, C_ in ((1, 1), (2, 3)):  # one record; six equal ones
            moving = np.broadcast_to(m, (steps, C_) + f.shape)
            mean, m2, count = (t.cpu().numpy() for t in run(f, moving, labels, spacing, fresh_state(f.shape, ~on)))
            assert np.array_equal(count[on], np.full(on.sum(), steps * C_))
            assert np.array_equal(mean[on].view(np.int32), np.full(on.sum(), want).view(np.int32)) and not m2[on].any()
            assert (count[~on] == -3).all() and (mean[~on] == 7.5).all() and (m2[~on] == -2.25).all()
    assert cases[0][2] > 0 and cases[1][2] < 0 < cases[2][2]  # the sign convention


# ------------------------------------------------------------------------------------------------ restatement parity
def longest_box_lines(fixed, moving, labels):
    """(ny, nz, nx) of the widest box of a (chain, label) pair: the voxels of the label in the fixed or the chain's map"""
    best = np.zeros(3, int)
    for step in moving:
        for m in step:
            for lab in labels:
                zyx = np.argwhere((fixed == lab) | (m == lab))
                if len(zyx):
                    ext = zyx.max(0) - zyx.min(0) + 1
                    best = np.maximum(best, [ext[1], ext[0], ext[2]])
    return best


@pytest.mark.parametrize('dims', SP.SHAPES)
@pytest.mark.parametrize('C_', SP.CHAINS)
def test_restatement_parity(dims, C_):
    fixed, moving, mask = SP.case_maps(dims, C_)
    ny, nz, nx = longest_box_lines(fixed, moving, SP.LABELS3)
    if dims == (9, 11, 70):
        assert nx > 64  # wider than one 64-lane chunk
    if dims == (70, 9, 5):
        assert nz > 64  # pass D keeps its envelopes in global scratch
    if dims == (3, 70, 6):
        assert ny > 64  # pass H does
    off = SP.fixed_contours(fixed, SP.LABELS3) < 0
    for spacing in SP.SPACINGS:
        ref = SP.case_reference(dims, C_, spacing)
        name = f'surface_posterior/{dims}/C{C_}/{spacing}'
        assert (ref['count'] >= 2).any()
        state = run(fixed, moving, SP.LABELS3, spacing, fresh_state(dims, off))
        mean, m2, count = (t.cpu().numpy() for t in state)
        assert (count[off] == -3).all() and (mean[off] == 7.5).all() and (m2[off] == -2.25).all()
        count_on = np.where(off, 0, count)
        SP.check_state(name, check, mean, m2, count_on, ref, ref['S'])
        # the float32 evaluation of the same recurrence in the same order: the device must reproduce it bit for bit
        m32, s32, _ = SP.welford(ref['s'], np.float32)
        on = ~off
        assert np.array_equal(mean[on].view(np.int32), m32[on].view(np.int32)) and np.array_equal(m2[on].view(np.int32), s32[on].view(np.int32))
        # the maps and the summary from a state that is zero off the contours, as a recorder's is
        clean = [dev(np.where(off, 0, a).astype(a.dtype)) for a in (mean, m2, count)]
        for mk in (None, mask):
            bias, std, isum, fsum = finalize(fixed, SP.LABELS3, clean, LEVELS, mk)
            SP.check_maps(name, check, bias, std, ref, ref['S'])
            assert np.isnan(bias[off]).all() and np.isnan(std[off]).all()
            SP.check_summary(name, check, isum, fsum, bias, std, ref, fixed, SP.LABELS3, LEVELS, ref['S'], mk)


def test_label_missing_from_one_chain_at_one_step():
    """the counts on that label's fixed contour advance by C - 1 at that step, and nothing else differs from the restatement"""
    dims, C_, spacing = (9, 11, 70), 3, ANISO
    fixed, moving, _ = SP.case_maps(dims, C_)
    lab = SP.LABELS3[1]
    gone = np.array(moving)
    gone[1, 0][gone[1, 0] == lab] = 0
    s = [SP.samples(fixed, gone[t], SP.LABELS3, spacing) for t in range(SP.STEPS)]
    mean64, m264, count64 = SP.welford(s, np.float64)
    full = SP.case_reference(dims, C_, spacing)
    li = SP.fixed_contours(fixed, SP.LABELS3)
    assert (li == 1).any() and np.array_equal(count64[li == 1], full['count'][li == 1] - 1)
    assert np.array_equal(count64[li != 1], full['count'][li != 1])
    mean, m2, count = (t.cpu().numpy() for t in run(fixed, gone, SP.LABELS3, spacing))
    ref = {'mean': mean64, 'm2': m264, 'count': count64}
    SP.check_state('surface_posterior/missing_label', check, mean, m2, count, ref, float(np.nanmax(np.abs(np.stack(s)))))
    m32, s32, _ = SP.welford(s, np.float32)
    assert np.array_equal(mean.view(np.int32), m32.view(np.int32)) and np.array_equal(m2.view(np.int32), s32.view(np.int32))


def test_label_missing_from_the_fixed_map():
    """no contour voxel: zero counts, and a NaN row in the summary of the recorder"""
    dims, C_ = (5, 7, 9), 2
    fixed, moving, _ = SP.case_maps(dims, C_)
    labels = SP.LABELS3 + [77]
    with_77 = np.array(moving)
    with_77[:, :, 2:4, 2:4, 2:4] = 77  # present in every moving map, never in the fixed one
    state = run(fixed, with_77, labels, ANISO)
    _, _, isum, fsum = finalize(fixed, labels, state)
    assert not isum[3].any() and np.array_equal(fsum[3], [0.0, 0.0, 0.0, -math.inf, 0.0, -math.inf])
    assert isum[:3, 0].all()
    sp = SurfacePosterior(dev(fixed), dict(a=10, b=16, c=58, absent=77), ANISO, DEV)
    for step in with_77:
        sp.record(dev(step)[:, None])
    assert sp.records == SP.STEPS * C_
    _, _, summary = sp.finalize()
    row = summary['structures']['absent']
    assert (row['contour_voxels'], row['sampled_voxels'], row['spread_voxels']) == (0, 0, 0)
    assert all(math.isnan(v) for k, v in row.items() if not k.endswith('_voxels'))
    assert all(math.isfinite(v) for v in summary['structures']['a'].values())


def test_64_labels_in_one_call():
    dims, C_ = (5, 7, 9), 2
    fixed, moving, mask = SP.case_maps(dims, C_)
    many = SP.LABELS3 + [l for l in range(100, 200)][:L.IRS_MAX_LABELS - len(SP.LABELS3)]
    assert len(many) == L.IRS_MAX_LABELS
    few_state, many_state = run(fixed, moving, SP.LABELS3, ANISO), run(fixed, moving, many, ANISO)
    for a, b in zip(few_state, many_state):
        assert torch.equal(a, b)
    few, lots = finalize(fixed, SP.LABELS3, few_state, LEVELS, mask), finalize(fixed, many, many_state, LEVELS, mask)
    assert np.array_equal(few[0], lots[0], equal_nan=True) and np.array_equal(few[1], lots[1], equal_nan=True)
    assert np.array_equal(few[2], lots[2][:3]) and np.array_equal(few[3], lots[3][:3]) and few[2][:, 2].all()
    assert not lots[2][3:].any() and (lots[3][3:] == np.array([0.0, 0.0, 0.0, -math.inf, 0.0, -math.inf])).all()


def test_two_runs_are_bit_identical():
    dims, C_ = (9, 11, 70), 3
    fixed, moving, mask = SP.case_maps(dims, C_)
    a, b = run(fixed, moving, SP.LABELS3, ANISO), run(fixed, moving, SP.LABELS3, ANISO)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    fa, fb = finalize(fixed, SP.LABELS3, a, LEVELS, mask), finalize(fixed, SP.LABELS3, b, LEVELS, mask)
    for x, y in zip(fa, fb):
        assert np.array_equal(x.view(np.int32 if x.dtype == np.float32 else np.int64), y.view(np.int32 if y.dtype == np.float32 else np.int64))


def test_agrees_with_the_directed_average_of_the_hausdorff_call():
    """after one step of one chain the mean over a structure's fixed contour of |s| is the A -> B half of the ASD: the same
    distances, one float32 rounding each"""
    dims = (9, 11, 70)
    fixed, moving, _ = SP.case_maps(dims, 1)
    lib = L.load()
    spacing = (0.7, 1.3, 2.1)
    f, m = dev(fixed)[None, None], dev(moving[0])[:, None]
    n = len(SP.LABELS3)
    lab = (C.c_int32 * n)(*SP.LABELS3)
    boxes = torch.empty((n, 6), device=DEV, dtype=torch.int32)
    L.check(lib.irs_label_boxes(L.dev_ptr(f), 1, L.dev_ptr(m), lab, n, L.dev_ptr(boxes), 1, *dims, L.stream_ptr()))
    boxes_h = boxes.cpu()
    bp = C.cast(C.c_void_p(boxes_h.data_ptr()), C.POINTER(C.c_int32))
    nbytes = C.c_size_t()
    L.check(lib.irs_hausdorff_workspace(bp, n, 0, *dims, C.byref(nbytes)))
    own = C.c_size_t()
    L.check(lib.irs_surface_posterior_workspace(bp, n, *dims, C.byref(own)))
    assert own.value == nbytes.value  # the surface posterior lives in the workspace of the Hausdorff call without percentiles
    ws = torch.empty(nbytes.value, device=DEV, dtype=torch.uint8)
    counts = torch.empty((n, 2), device=DEV, dtype=torch.int64)
    sums, hd = torch.empty((n, 2), device=DEV, dtype=torch.float64), torch.empty((n, 2), device=DEV, dtype=torch.float64)
    L.check(lib.irs_label_hausdorff_distance(L.dev_ptr(f), 1, L.dev_ptr(m), lab, n, (C.c_float * 3)(*spacing), bp, L.dev_ptr(ws),
                                             nbytes.value, None, 0, L.dev_ptr(counts), L.dev_ptr(sums), L.dev_ptr(hd), None, 1, *dims,
                                             L.stream_ptr()))
    state = run(fixed, moving[:1], SP.LABELS3, spacing)
    _, _, isum, fsum = finalize(fixed, SP.LABELS3, state)
    counts, sums, hd = counts.cpu().numpy(), sums.cpu().numpy(), hd.cpu().numpy()
    assert (counts > 0).all() and np.array_equal(isum[:, 0], counts[:, 0]) and np.array_equal(isum[:, 1], counts[:, 0])
    np.testing.assert_allclose(fsum[:, 1] / isum[:, 1], sums[:, 0] / counts[:, 0], rtol=1e-6)
    np.testing.assert_allclose(fsum[:, 3], hd[:, 0], rtol=1e-6)  # and the largest |s| is the directed Hausdorff distance


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize('fn,bad,message', SP.abi_refusals())
def test_abi_refusals(fn, bad, message):
    SP.assert_refused(fn, bad, message)


def test_python_refusals():
    dims = (4, 5, 6)
    f = torch.zeros((1, 1) + dims, dtype=torch.int16, device=DEV)
    m = torch.zeros((2, 1) + dims, dtype=torch.int16, device=DEV)
    state = lambda: fresh_state(dims)
    good = dict(seg_fixed=f, seg_moving=m, labels=[10, 16], spacing=(1.0, 1.0, 1.0))
    bad = [dict(seg_fixed=f.cpu()), dict(seg_moving=m.cpu()), dict(seg_fixed=f.float()), dict(seg_moving=m.int()),
           dict(seg_fixed=torch.zeros((2, 1) + dims, dtype=torch.int16, device=DEV)), dict(seg_fixed=f[:, :, :3]),
           dict(seg_moving=torch.zeros((9, 1) + dims, dtype=torch.int16, device=DEV)), dict(labels=[]), dict(labels=list(range(65))),
           dict(labels=[10, 10]), dict(labels=[40000]), dict(spacing=(1.0, 0.0, 1.0)), dict(spacing=(1.0, float('inf'), 1.0)),
           dict(spacing=(1.0, float('nan'), 1.0)), dict(spacing=(1.0, 1.0))]
    for kw in bad:
        with pytest.raises(L.IrsError):
            ops.surface_posterior_update(**{**good, **kw}, **dict(zip(('mean', 'm2', 'count'), state())))
    for j, wrong in enumerate((lambda t: t.cpu(), lambda t: t.double(), lambda t: t[:3])):
        for i in range(3):
            st = list(state())
            st[i] = wrong(st[i])
            with pytest.raises(L.IrsError):
                ops.surface_posterior_update(**good, mean=st[0], m2=st[1], count=st[2])
            with pytest.raises(L.IrsError):
                ops.surface_posterior_finalize(f, [10, 16], *st, LEVELS)
    for kw in (dict(levels=(0.0,)), dict(levels=(1.0,)), dict(levels=(0.9, 0.5)), dict(levels=(0.5, 0.5)), dict(levels=(0.1, 0.2, 0.3, 0.4, 0.5)),
               dict(levels=(float('nan'),)), dict(labels=[10, 10]), dict(labels=[]), dict(seg_fixed=f.cpu()), dict(seg_fixed=f[0]),
               dict(mask=torch.ones((4, 5, 7), dtype=torch.bool, device=DEV)), dict(mask=torch.ones(dims, device=DEV))):
        args = dict(seg_fixed=f, labels=[10, 16], levels=LEVELS, mask=None)
        args.update(kw)
        with pytest.raises(L.IrsError):
            ops.surface_posterior_finalize(args['seg_fixed'], args['labels'], *state(), args['levels'], args['mask'])
    # and the calls still work afterwards: nothing to record, nothing touched
    st = state()
    ops.surface_posterior_update(**good, mean=st[0], m2=st[1], count=st[2])
    bias, std, isum, fsum = ops.surface_posterior_finalize(f, [10, 16], *st, ())
    assert not st[2].any() and torch.isnan(bias).all() and torch.isnan(std).all() and not isum.any()
    with pytest.raises(ValueError, match='surface posterior'):
        SurfacePosterior(f, dict(a=1, b=1), (1, 1, 1), DEV)
    with pytest.raises(ValueError, match='surface posterior'):
        SurfacePosterior(f, dict(a=1), (1, 0, 1), DEV)
    with pytest.raises(ValueError, match='surface posterior'):
        SurfacePosterior(f.float(), dict(a=1), (1, 1, 1), DEV)
    sp = SurfacePosterior(f, dict(a=1), (1, 1, 1), DEV)
    with pytest.raises(RuntimeError, match='nothing recorded'):
        sp.finalize()
    sd = sp.state_dict()
    with pytest.raises(ValueError, match='labels'):
        SurfacePosterior(f, dict(a=2), (1, 1, 1), DEV).load_state_dict(sd)
    with pytest.raises(ValueError, match='shape'):
        SurfacePosterior(f[:, :, :3], dict(a=1), (1, 1, 1), DEV).load_state_dict(sd)


def test_calc_surface_posterior_and_the_recorder_state():
    from ir_sgmcmc_amd.utils import calc_surface_posterior
    dims, C_ = (5, 7, 9), 2
    fixed, moving, mask = SP.case_maps(dims, C_)
    structures = dict(a=10, b=16, c=58)
    samples = dev(moving).permute(1, 0, 2, 3, 4)[:, :, None].contiguous()  # (C, N, 1, D, H, W)
    bias, std, summary = calc_surface_posterior(dev(fixed), samples, structures, ANISO, dev(mask), LEVELS)
    state = run(fixed, moving, SP.LABELS3, ANISO)
    b2, s2, isum, fsum = ops.surface_posterior_finalize(dev(fixed)[None, None], SP.LABELS3, *state, LEVELS, dev(mask))
    assert torch.equal(bias.view(torch.int32), b2.view(torch.int32)) and torch.equal(std.view(torch.int32), s2.view(torch.int32))
    assert summary['records'] == SP.STEPS * C_
    for j, name in enumerate(structures):
        st = summary['structures'][name]
        assert st['contour_voxels'] == int(isum[j, 0]) and st['bias'] == float(fsum[j, 0]) / int(isum[j, 1])
        assert st['coverage_90'] == int(isum[j, 4]) / int(isum[j, 2]) and st['max_std'] == float(fsum[j, 5])
    # a recorder restored from its state_dict continues bit for bit
    a = SurfacePosterior(dev(fixed), structures, ANISO, DEV)
    a.record(dev(moving[0])[:, None])
    b = SurfacePosterior(dev(fixed), structures, ANISO, DEV)
    b.load_state_dict(a.state_dict())
    for sp in (a, b):
        for step in moving[1:]:
            sp.record(dev(step)[:, None])
    assert b.records == a.records == SP.STEPS * C_
    for x, y, z in zip((a.mean, a.m2, a.count), (b.mean, b.m2, b.count), state):
        assert torch.equal(x, y) and torch.equal(x, z)


# ------------------------------------------------------------------------------------------------ the trainer option
N = 16


def make_trainer(tmp_path, **trainer_over):
    from ir_sgmcmc_amd.parse_config import ConfigParser
    from ir_sgmcmc_amd.trainer import Trainer
    cfg = json.load(open(os.path.join(ROOT, 'configs', 'synthetic_gmm_lognormal.json')))
    cfg['trainer'].update(save_dir=str(tmp_path), **trainer_over)
    cfg['data_loader']['args']['dims'] = [N, N, N]
    config = ConfigParser.from_dict(copy.deepcopy(cfg), timestamp='t')
    tm, rm = config.init_transformation_and_registration_modules()
    return Trainer(config, config.init_data_loader(), config.init_losses(), tm, rm, config.init_metrics(), device=DEV)


def test_trainer_maps_match_the_recorded_warps(tmp_path, monkeypatch):
    from ir_sgmcmc_amd.utils.imageio import read_nifti
    kept = []
    record = SurfacePosterior.record

    def spy(self, seg_warped):
        kept.append(seg_warped.clone())
        return record(self, seg_warped)

    monkeypatch.setattr(SurfacePosterior, 'record', spy)
    kw = dict(no_iters_burn_in=3, no_samples_MCMC=9, log_period_MCMC=4)
    torch.manual_seed(0)
    t = make_trainer(tmp_path / 'on', surface_posterior={'period': 2, 'coverage': [0.5, 0.9]}, **kw)
    t.run()
    monkeypatch.setattr(SurfacePosterior, 'record', record)
    C_ = t.no_chains
    assert len(kept) == len(recorded_steps(3, 9, 2)) == 9 // 2 and t._surface_posterior.records == C_ * (9 // 2)
    fixed_data = next(iter(t.data_loader))[0]
    spacing = t.data_loader.im_spacing if getattr(t.data_loader, 'im_spacing', None) is not None else torch.ones(3)
    again = SurfacePosterior(fixed_data['seg'], t.structures_dict, spacing, DEV)
    for seg in kept:
        again.record(seg)
    bias, std, summary = again.finalize(fixed_data['mask'][0], (0.5, 0.9))
    assert torch.equal(bias.view(torch.int32), t.surface_bias.view(torch.int32))
    assert torch.equal(std.view(torch.int32), t.surface_std.view(torch.int32))
    assert json.dumps(summary, sort_keys=True) == json.dumps(t.surface_summary, sort_keys=True)  # NaN == NaN as text
    seen = [s for s, st in summary['structures'].items() if st['spread_voxels']]
    seg_fixed = fixed_data['seg'].reshape(N, N, N).numpy()
    present = {s for s, lab in t.structures_dict.items() if (seg_fixed == lab).any()}  # the structures of the synthetic label map
    assert set(seen) == present and {'left_thalamus', 'brain_stem'} <= present and 'left_caudate' not in present
    # files: NaN off the contours
    folder = t.config.save_dirs['samples']
    on = SP.fixed_contours(seg_fixed, list(t.structures_dict.values())) >= 0
    for name, want in (('MCMC_surface_bias', t.surface_bias), ('MCMC_surface_std', t.surface_std)):
        im, _ = read_nifti(str(folder / f'{name}.nii.gz'))
        assert np.array_equal(im, want.cpu().numpy(), equal_nan=True)
        assert np.isnan(im[~on]).all() and np.isfinite(im[on]).all()
    # metrics
    res = t.metrics.result()
    names = surface_metric_names(t.surface_options, t.structures_dict)
    assert len(names) == 5 * len(t.structures_dict) and 'MCMC/surface/coverage_90/brain_stem' in names
    for key in names:
        _, _, k, s = key.split('/')
        got, want = res[key], summary['structures'][s][k]
        assert (math.isnan(got) and math.isnan(want)) or got == want, key
    assert math.isfinite(res['MCMC/surface/bias/brain_stem']) and math.isnan(res['MCMC/surface/bias/left_caudate'])
    # the same run with the option off: the same outputs, no surface anything
    torch.manual_seed(0)
    off = make_trainer(tmp_path / 'off', **kw)
    off.run()
    assert torch.equal(off.displacement_mean, t.displacement_mean) and torch.equal(off.displacement_std, t.displacement_std)
    assert off.surface_bias is None and off.surface_std is None and off.surface_summary is None
    res_off = off.metrics.result()
    assert list(res_off) == [k for k in res if k not in names]
    assert not list(off.config.save_dirs['samples'].glob('*surface*'))
    assert sorted(p.name for p in off.config.save_dirs['samples'].glob('*')) == \
        sorted(p.name for p in folder.glob('*') if 'surface' not in p.name)


def test_trainer_surface_posterior_survives_checkpoint_resume_bit_for_bit(tmp_path):
    kw = dict(no_iters_burn_in=2, no_samples_MCMC=8, log_period_MCMC=4, checkpoint_period=6, surface_posterior={'period': 2},
              save_outputs=False)
    a = make_trainer(tmp_path / 'a', **kw)
    a.run()
    ck = a.config.save_dirs['checkpoints'] / 'checkpoint_0000006.pt'
    sd = torch.load(ck, map_location='cpu', weights_only=True)
    assert sd['surface_posterior']['records'] == 2 * a.no_chains and sd['surface_posterior']['labels'] == list(a.structures_dict.values())
    b = make_trainer(tmp_path / 'b', resume=str(ck), **kw)
    b.run()
    for name in ('mean', 'm2', 'count'):
        assert torch.equal(getattr(a._surface_posterior, name), getattr(b._surface_posterior, name)), name
    assert a._surface_posterior.records == b._surface_posterior.records == 4 * a.no_chains
    assert torch.equal(a.surface_bias.view(torch.int32), b.surface_bias.view(torch.int32))
    assert torch.equal(a.surface_std.view(torch.int32), b.surface_std.view(torch.int32))
    assert json.dumps(a.surface_summary, sort_keys=True) == json.dumps(b.surface_summary, sort_keys=True)
    assert not list(a.config.save_dirs['samples'].glob('*surface*'))  # save_outputs off
    # a checkpoint without the key, once a recorded step has passed, is refused; the option off keeps the key set
    del sd['surface_posterior']
    ck2 = tmp_path / 'no_surface.pt'
    torch.save(sd, ck2)
    c = make_trainer(tmp_path / 'c', resume=str(ck2), **kw)
    with pytest.raises(ValueError, match='surface_posterior'):
        c.run()
    off = make_trainer(tmp_path / 'off', **{k: v for k, v in kw.items() if k != 'surface_posterior'})
    off.run()
    sd_off = torch.load(off.config.save_dirs['checkpoints'] / 'checkpoint_0000006.pt', map_location='cpu', weights_only=True)
    assert set(sd_off) == set(sd)
