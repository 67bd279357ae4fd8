"""Displacement credible intervals on the device: the histogram against the numpy restatement as integers, the quantile maps,
the width map and the summary against the restatement of the device's own histogram, the quantiles against numpy.sort (the
one-bin bound, at every voxel), clipping, NaN inputs, launch equivalence and determinism, the count ceiling, the ABI and Python
refusals, and the trainer option end to end (maps against the recorded displacements, files, metrics, checkpoint / resume, and
nothing changed when it is off).

tests/_displacement_quantiles.py holds the restatement, the inputs and the tolerance; test_displacement_quantiles_host.py
checks on the CPU that the restatement itself keeps the bound and that the in-range cases are in range.

Measured on one MI355X, worst over all cases: histogram and centre equal to the restatement everywhere; maps against the
restatement of the device's histogram 1.2e-7 relative (tolerance 1e-6); quantile against the order statistic 0.9999991 of the
tolerance (a quantile may sit at one end of its bin and the order statistic at the other).  Update 0.81 ms and finalize
4.19 ms at 256^3 with 2 chains and 64 bins."""
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
from ir_sgmcmc_amd.diagnostics import QUANTILE_METRICS, DisplacementQuantiles, recorded_steps
from ir_sgmcmc_amd.parse_config import ConfigParser
from ir_sgmcmc_amd.trainer import Trainer
from ir_sgmcmc_amd.utils import calc_displacement_quantiles
from tests._displacement_quantiles import (BIN_WIDTH, CASES, CLIP_CASE, CLIP_NOISE, HAND_BIN_WIDTH, HAND_CI, HAND_OFFSETS,
                                           HAND_PROBS, HAND_SCALE, IN_RANGE_CASES, PROBS, case_mask, case_seed, check_bound,
                                           check_monotone, draw_records, finalize_np, hand_checked_records, quantiles_np,
                                           summary_np)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_KEYS = ('records', 'voxels', 'out_of_range_voxels', 'clipped_samples')
FLOAT_KEYS = ('width_mean', 'width_max', 'width_x', 'width_y', 'width_z', 'out_of_range_frac', 'clipped_frac')


def hist_np(dq):
    return dq.hist.cpu().numpy().astype(np.int64)


def run_device(records, C, probs=PROBS, mask=None, bins=64, bin_width=BIN_WIDTH, scale=None):
    """records (n,3,D,H,W) float32 in record order, C chains per step -> (DisplacementQuantiles, quantiles, ci_width as
    numpy, summary)"""
    n = records.shape[0]
    assert n % C == 0
    dq = DisplacementQuantiles(records.shape[2:], DEV, bins, bin_width, scale)
    rec = torch.from_numpy(records).to(DEV)
    for s in range(n // C):
        dq.record(rec[s * C:(s + 1) * C].contiguous())
    m = None if mask is None else torch.from_numpy(mask).to(DEV)
    q, ci, summary = dq.finalize(probs, m)
    return dq, q.cpu().numpy(), ci.cpu().numpy(), summary


def check_state(dq, ref):
    """centre bit for bit, every count of every bin as an integer"""
    assert np.array_equal(dq.centre.cpu().numpy().view(np.int32), ref['centre'].view(np.int32))
    h = hist_np(dq)
    assert h.shape == ref['hist'].shape and np.array_equal(h, ref['hist'])
    assert np.array_equal(dq.histogram().cpu().numpy(), ref['hist'])
    assert [float(w) for w in dq.width] == ref['width'].tolist() and [float(w) for w in dq.inv_width] == ref['inv_width'].tolist()


def check_outputs(dq, q, ci, summary, probs, mask):
    """quantiles, ci_width and summary against the restatement evaluated on the DEVICE's histogram: floats to 1e-6 relative,
    integers and the NaN pattern exactly"""
    want_q, want_ci = finalize_np(dq.centre.cpu().numpy(), hist_np(dq), dq.records, np.array(dq.width), dq.scale, probs)
    worst = 0.0
    for got, want in ((q, want_q), (ci, want_ci)):
        assert got.dtype == np.float32 and got.shape == want.shape
        assert np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        err = np.abs(got[ok].astype(np.float64) - want[ok]) / np.maximum(np.abs(want[ok].astype(np.float64)), 1e-300)
        worst = max(worst, float(err.max()) if err.size else 0.0)
        assert (np.abs(got[ok].astype(np.float64) - want[ok]) <= 1e-6 * np.abs(want[ok])).all()
    want = summary_np(dq.records, hist_np(dq), q, ci, mask)  # of the device's stored maps: this pins the reduction
    for key in INT_KEYS:
        assert summary[key] == want[key], (key, summary[key], want[key])
    for key in FLOAT_KEYS:
        g, w = summary[key], want[key]
        assert (math.isnan(g) and math.isnan(w)) or abs(g - w) <= 1e-6 * abs(w), (key, g, w)
    print({'maps against the restatement, worst relative error': worst})


def test_hand_checked_case():
    records, centre = hand_checked_records()
    dq, q, ci, s = run_device(records, 2, HAND_PROBS, bins=8, bin_width=HAND_BIN_WIDTH, scale=HAND_SCALE)
    h = hist_np(dq)
    assert dq.records == 4 and (h[:, 4] == 2).all() and (h[:, 5] == 2).all() and h.sum() == 4 * centre.size
    for j, off in enumerate(HAND_OFFSETS):
        assert np.array_equal(q[j], (2.0 * (centre + off)).astype(np.float32))
    assert np.array_equal(ci, np.full(centre.shape[1:], HAND_CI, dtype=np.float32))
    assert (s['records'], s['voxels'], s['out_of_range_voxels'], s['clipped_samples']) == (4, 60, 0, 0)
    assert s['width_mean'] == pytest.approx(HAND_CI, rel=1e-6) and s['width_max'] == pytest.approx(HAND_CI, rel=1e-6)
    assert s['width_x'] == s['width_y'] == s['width_z'] == 1.0 and s['out_of_range_frac'] == 0.0 and s['clipped_frac'] == 0.0
    check_state(dq, quantiles_np(records, HAND_PROBS, bins=8, bin_width=HAND_BIN_WIDTH, scale=HAND_SCALE))


@pytest.mark.parametrize('with_mask', [False, True])
@pytest.mark.parametrize('C,steps,shape,bins', CASES)
def test_histogram_parity_and_the_maps(C, steps, shape, bins, with_mask):
    n = C * steps
    records = draw_records(n, shape, case_seed(C, steps, shape, bins))
    mask = case_mask(shape) if with_mask else None
    dq, q, ci, s = run_device(records, C, mask=mask, bins=bins)
    assert dq.records == n
    ref = quantiles_np(records, PROBS, bins=bins, mask=mask)
    check_state(dq, ref)
    check_outputs(dq, q, ci, s, PROBS, mask)
    check_monotone(q)
    assert np.array_equal(np.isnan(q), np.isnan(ref['quantiles']))


@pytest.mark.parametrize('C,steps,shape,bins', IN_RANGE_CASES)
def test_in_range_quantiles_are_within_a_bin_of_the_order_statistic(C, steps, shape, bins):
    n = C * steps
    records = draw_records(n, shape, case_seed(C, steps, shape, bins))
    dq, q, ci, s = run_device(records, C, bins=bins)
    check_state(dq, quantiles_np(records, PROBS, bins=bins))
    assert s['out_of_range_voxels'] == 0 and s['voxels'] == int(np.prod(shape)) and np.isfinite(q).all() and np.isfinite(ci).all()
    check_bound(records, PROBS, q, BIN_WIDTH, dq.scale)  # every voxel, every channel, every probability
    check_monotone(q)
    check_outputs(dq, q, ci, s, PROBS, None)
    more = (0.01, 0.05, 0.25, 0.5, 0.75, 0.9, 0.95, 0.99)  # the most probabilities one call takes
    q8, ci8, s8 = dq.finalize(more)
    q8, ci8 = q8.cpu().numpy(), ci8.cpu().numpy()
    check_outputs(dq, q8, ci8, s8, more, None)
    check_monotone(q8)
    check_bound(records, more, q8, BIN_WIDTH, dq.scale, where=np.isfinite(q8).all(axis=0))
    assert np.array_equal(q8[1], q[0]) and np.array_equal(q8[3], q[1]) and np.array_equal(q8[6], q[2])


# 263 blocks of partials: threads 0 .. 6 of the second stage fold two blocks each, and V % 256 != 0; 270 400 voxels: more than
# 1024 blocks x 256, so the first stage's grid-stride loop wraps, with a ragged tail.  The smallest shapes on either path.
@pytest.mark.parametrize('shape', [(41, 40, 41), (65, 64, 65)])
def test_summary_reduction_past_one_round_of_either_stage(shape):
    """the summary against the restatement of the DEVICE's stored maps and histogram, as check_outputs pins the reduction.
    16 bins (29 MB of state at the larger shape) of 0.125 voxels reach 0.875 voxels either side of the centre; with noise of
    0.75 voxels the restatement has about 86 % of the voxels in range, so no column of the summary is empty"""
    records = draw_records(3, shape, case_seed(3, 1, shape, 16), noise=0.75)
    dq = DisplacementQuantiles(shape, DEV, 16, BIN_WIDTH)
    dq.record(torch.from_numpy(records).to(DEV).contiguous())
    for mask in (case_mask(shape), None):
        ref = quantiles_np(records, PROBS, bins=16, mask=mask)['summary']
        assert 0 < 2 * ref['out_of_range_voxels'] <= ref['voxels'] and ref['clipped_samples'] > 0  # a condition on the inputs
        q, ci, summary = dq.finalize(PROBS, None if mask is None else torch.from_numpy(mask).to(DEV))
        want = summary_np(3, hist_np(dq), q.cpu().numpy(), ci.cpu().numpy(), mask)
        print({key: (summary[key], want[key]) for key in INT_KEYS + FLOAT_KEYS})
        for key in INT_KEYS:
            assert summary[key] == want[key], (key, summary[key], want[key])
        for key in FLOAT_KEYS:
            g, w = summary[key], want[key]
            assert (math.isnan(g) and math.isnan(w)) or abs(g - w) <= 1e-6 * abs(w), (key, g, w)


def test_the_clipping_case():
    Cn, steps, shape, bins = CLIP_CASE
    n = Cn * steps
    records = draw_records(n, shape, case_seed(*CLIP_CASE), noise=CLIP_NOISE)
    mask = case_mask(shape)
    dq, q, ci, s = run_device(records, Cn, mask=mask, bins=bins)
    ref = quantiles_np(records, PROBS, bins=bins, mask=mask)
    check_state(dq, ref)
    assert np.array_equal(np.isnan(q), np.isnan(ref['quantiles'])) and np.array_equal(np.isnan(ci), np.isnan(ref['ci_width']))
    bad = np.isnan(q).any(axis=(0, 1))
    assert 0 < (bad & mask).sum() < mask.sum()
    assert s['out_of_range_voxels'] == ref['summary']['out_of_range_voxels'] == int((bad & mask).sum())
    assert s['clipped_samples'] == ref['summary']['clipped_samples'] > 0
    check_outputs(dq, q, ci, s, PROBS, mask)
    check_monotone(q)
    for j in range(len(PROBS)):  # whatever is in range still holds the bound
        check_bound(records, PROBS[j:j + 1], q[j:j + 1], BIN_WIDTH, dq.scale, where=np.isfinite(q[j]))


def test_nan_inputs_and_an_empty_mask():
    shape = (4, 5, 6)
    records = draw_records(8, shape, 4)
    clean = records.copy()
    records[3, 2, 1, 2, 3] = np.nan   # one record of eight: one count in bin 0 of that voxel and channel
    records[0, 1, 3, 4, 5] = np.nan   # in the first record: the centre is NaN and every record of that voxel counts into bin 0
    dq, q, ci, s = run_device(records, 2)
    ref = quantiles_np(records, PROBS)
    check_state(dq, ref)
    h = hist_np(dq)
    assert h[2, 0, 1, 2, 3] == 1 and h[1, 0, 3, 4, 5] == 8
    assert np.isnan(q[:, 1, 3, 4, 5]).all() and np.isnan(ci[3, 4, 5]) and np.isfinite(q[:, 0, 3, 4, 5]).all()
    assert np.isnan(q[0, 2, 1, 2, 3]) and np.isfinite(q[1:, 2, 1, 2, 3]).all()  # r = 0.4 falls into bin 0, the others do not
    assert s['out_of_range_voxels'] == 2 and s['clipped_samples'] == 9
    _, q0, ci0, _ = run_device(clean, 2)
    same = np.ones(q.shape, dtype=bool)
    same[:, 1, 3, 4, 5] = False
    same[:, 2, 1, 2, 3] = False
    assert np.array_equal(q[same], q0[same])  # the neighbours are what they are without the NaNs
    check_outputs(dq, q, ci, s, PROBS, None)
    m = torch.zeros(shape, dtype=torch.bool, device=DEV)
    _, _, s0 = dq.finalize(PROBS, m)
    assert s0['voxels'] == 0 and all(math.isnan(s0[k]) for k in FLOAT_KEYS)
    m[3, 4, 5] = True
    _, _, s1 = dq.finalize(PROBS, m)  # no masked voxel is in range
    assert s1['voxels'] == 1 and s1['out_of_range_frac'] == 1.0 and s1['clipped_samples'] == 8 and math.isnan(s1['width_mean'])
    assert math.isnan(s1['width_max'])


@pytest.mark.parametrize('shape', [(5, 7, 9), (3, 5, 131)])
def test_launch_equivalence_and_determinism(shape):
    records = draw_records(11, shape, 5)  # more records than one launch takes
    t = torch.from_numpy(records).to(DEV)
    q, ci, s = calc_displacement_quantiles(t)
    assert s['records'] == 11
    one = DisplacementQuantiles(shape, DEV)
    one.centre.fill_(3.0)  # records_before = 0 overwrites whatever the state held
    one.hist.view(torch.int16).fill_(-7)
    for r in range(11):
        one.record(t[r:r + 1].contiguous())
    odd = DisplacementQuantiles(shape, DEV)
    for lo, hi in ((0, 3), (3, 4), (4, 11)):
        odd.record(t[lo:hi].contiguous())
    shuffled = DisplacementQuantiles(shape, DEV)  # the same first record, the others in another order
    order = [0] + (1 + np.random.default_rng(3).permutation(10)).tolist()
    for lo in range(0, 11, 4):
        shuffled.record(t[order[lo:lo + 4]].contiguous())
    ref = quantiles_np(records, PROBS)
    for other in (one, odd, shuffled):
        check_state(other, ref)
        out = other.finalize(PROBS)
        for got, want in zip(out[:2], (q, ci)):
            assert torch.equal(got.view(torch.int32), want.view(torch.int32))
        assert json.dumps(out[2], sort_keys=True) == json.dumps(s, sort_keys=True)
    # the functional form takes a mask, the bins and a scale
    mask = torch.from_numpy(case_mask(shape)).to(DEV)
    q2, _, s2 = calc_displacement_quantiles(t, (0.25, 0.75), mask, bins=32, bin_width=0.25, scale=(2.0, 2.0, 2.0))
    assert tuple(q2.shape) == (2, 3) + shape and s2['voxels'] == int(mask.sum())


def test_two_runs_and_two_finalize_calls_are_bit_identical():
    shape = (13, 17, 19)  # more than one block of partials
    records = draw_records(6, shape, 11)
    mask = np.random.default_rng(2).random(shape) < 0.3
    a = run_device(records, 3, mask=mask)
    b = run_device(records, 3, mask=mask)
    assert np.array_equal(hist_np(a[0]), hist_np(b[0])) and torch.equal(a[0].centre, b[0].centre)
    for x, y in zip(a[1:3], b[1:3]):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))
    assert json.dumps(a[3], sort_keys=True) == json.dumps(b[3], sort_keys=True)
    check_outputs(a[0], a[1], a[2], a[3], PROBS, mask)
    m = torch.from_numpy(mask).to(DEV)
    dq = a[0]
    r1 = ops.displacement_quantiles_finalize(dq.centre, dq.hist, 6, dq.width, dq.scale, PROBS, m)
    r2 = ops.displacement_quantiles_finalize(dq.centre, dq.hist, 6, dq.width, dq.scale, PROBS, m)
    for u, v in zip(r1, r2):
        assert torch.equal(u.view(torch.uint8), v.view(torch.uint8))
    assert r1[2].dtype == torch.int64 and int(r1[2][0]) == int(mask.sum()) and r1[3].dtype == torch.float64
    assert tuple(r1[2].shape) == (L.IRS_QUANTILE_SUMMARY_INTS,) and tuple(r1[3].shape) == (L.IRS_QUANTILE_SUMMARY_FLOATS,)


def test_the_count_ceiling():
    shape, B = (2, 3, 4), 8
    dq = DisplacementQuantiles(shape, DEV, bins=B, bin_width=1.0, scale=(1.0, 1.0, 1.0))
    hist = np.zeros((3, B) + shape, dtype=np.uint16)
    hist[:, B // 2] = 65534
    dq.load_state_dict({'centre': torch.zeros((3,) + shape), 'hist': torch.from_numpy(hist), 'records': 65534, 'bins': B,
                        'bin_width': 1.0})
    x = torch.full((1, 3) + shape, 0.5, device=DEV)
    dq.record(x)
    full = hist_np(dq)
    assert dq.records == 65535 and (full[:, B // 2] == 65535).all() and full.sum() == 65535 * 3 * 24
    q, ci, s = dq.finalize((0.25, 0.75))
    assert s['records'] == 65535 and torch.allclose(q[0], torch.full_like(q[0], 0.25)) and torch.allclose(q[1], torch.full_like(q[1], 0.75))
    with pytest.raises(ValueError, match='65535'):
        dq.record(x)
    with pytest.raises(L.IrsError):
        ops.displacement_quantiles_update(x, dq.centre, dq.hist, dq.inv_width, 65535)
    iw = (C.c_float * 3)(1.0, 1.0, 1.0)
    rc = L.load().irs_displacement_quantiles_update(C.c_void_p(x.data_ptr()), 1, *shape, C.c_void_p(dq.centre.data_ptr()),
                                                    C.c_void_p(dq.hist.data_ptr()), B, iw, 65535, L.stream_ptr())
    assert rc != 0 and b'65535' in L.load().irs_last_error()
    torch.cuda.synchronize()
    assert dq.records == 65535 and np.array_equal(hist_np(dq), full)


def test_abi_and_python_refusals():
    lib = L.load()
    Cn, D, H, W, B, P = 2, 4, 5, 6, 16, 3
    x = torch.from_numpy(draw_records(Cn, (D, H, W), 1)).to(DEV)
    centre = torch.zeros(3, D, H, W, device=DEV)
    hist = torch.zeros(3, B, D, H, W, device=DEV, dtype=torch.int16).view(torch.uint16)
    quant = torch.full((P, 3, D, H, W), -5.0, device=DEV)
    ciw = torch.full((D, H, W), -5.0, device=DEV)
    isum = torch.full((3,), -5, device=DEV, dtype=torch.int64)
    fsum = torch.full((5,), -5.0, device=DEV, dtype=torch.float64)
    ws = torch.empty(L.IRS_QUANTILE_WS_BYTES, device=DEV, dtype=torch.uint8)
    q = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    st = L.stream_ptr()
    f3 = lambda *v: (C.c_float * 3)(*v)
    dbl = lambda *v: (C.c_double * len(v))(*v)
    good = f3(1.0, 1.0, 1.0)
    bad_f3 = [f3(*s) for s in ((0.0, 1, 1), (1, -2.0, 1), (1, 1, float('nan')), (float('inf'), 1, 1))]

    def upd(x_=x, C_=Cn, D_=D, centre_=centre, hist_=hist, bins=B, iw=good, before=0):
        return lib.irs_displacement_quantiles_update(q(x_), C_, D_, H, W, q(centre_), q(hist_), bins, iw, before, st)

    def fin(centre_=centre, hist_=hist, bins=B, D_=D, n=2, width=good, scale=good, probs=dbl(0.05, 0.5, 0.95), P_=P, quant_=quant,
            ciw_=ciw, isum_=isum, fsum_=fsum, ws_=ws, ws_bytes=L.IRS_QUANTILE_WS_BYTES):
        return lib.irs_displacement_quantiles_finalize(q(centre_), q(hist_), bins, D_, H, W, n, width, scale, probs, P_, None,
                                                       q(quant_), q(ciw_), q(isum_), q(fsum_), q(ws_), ws_bytes, st)

    for kw in (dict(x_=None), dict(centre_=None), dict(hist_=None), dict(iw=None), dict(C_=0), dict(C_=9), dict(D_=1), dict(D_=0),
               dict(bins=15), dict(bins=2), dict(bins=0), dict(bins=258), dict(bins=-4), dict(before=-1), dict(before=65534),
               dict(before=2 ** 31 - 1), *(dict(iw=s) for s in bad_f3)):
        with pytest.raises(L.IrsError):
            L.check(upd(**kw))
    for kw in (dict(centre_=None), dict(hist_=None), dict(width=None), dict(scale=None), dict(probs=None), dict(quant_=None),
               dict(ciw_=None), dict(isum_=None), dict(fsum_=None), dict(ws_=None), dict(D_=1), dict(bins=15), dict(bins=2),
               dict(bins=258), dict(n=0), dict(n=-1), dict(n=65536), dict(P_=1), dict(P_=9), dict(P_=0), dict(ws_bytes=8),
               dict(ws_bytes=L.IRS_QUANTILE_WS_BYTES - 1), dict(probs=dbl(0.5, 0.5, 0.95)), dict(probs=dbl(0.5, 0.05, 0.95)),
               dict(probs=dbl(0.0, 0.5, 0.95)), dict(probs=dbl(0.05, 0.5, 1.0)), dict(probs=dbl(0.05, float('nan'), 0.95)),
               dict(probs=dbl(-0.1, 0.5, 0.95)), *(dict(width=s) for s in bad_f3), *(dict(scale=s) for s in bad_f3)):
        with pytest.raises(L.IrsError):
            L.check(fin(**kw))
    torch.cuda.synchronize()
    # nothing was counted or written by a refused call
    assert float(centre.abs().sum()) == 0.0 and not hist.cpu().numpy().any()
    assert bool((quant == -5).all()) and bool((ciw == -5).all()) and bool((isum == -5).all()) and bool((fsum == -5).all())
    L.check(upd())
    L.check(fin())
    torch.cuda.synchronize()
    assert int(isum[0]) == D * H * W and int(hist.cpu().numpy().astype(np.int64).sum()) == 2 * 3 * D * H * W
    # the Python surface checks dtypes, shapes, devices and values before it calls
    one, pr = (1.0, 1.0, 1.0), (0.05, 0.5, 0.95)
    for bad in (lambda: ops.displacement_quantiles_update(x.double(), centre, hist, one, 0),
                lambda: ops.displacement_quantiles_update(x.cpu(), centre, hist, one, 0),
                lambda: ops.displacement_quantiles_update(x[:, :2].contiguous(), centre, hist, one, 0),
                lambda: ops.displacement_quantiles_update(x[:, :, :2].contiguous(), centre, hist, one, 0),
                lambda: ops.displacement_quantiles_update(x, centre.double(), hist, one, 0),
                lambda: ops.displacement_quantiles_update(x, centre, hist.view(torch.int16), one, 0),
                lambda: ops.displacement_quantiles_update(x, centre, hist[:, :15], one, 0),
                lambda: ops.displacement_quantiles_update(x, centre, hist[:2], one, 0),
                lambda: ops.displacement_quantiles_update(x, centre, hist[0], one, 0),
                lambda: ops.displacement_quantiles_update(x, centre.cpu(), hist.cpu(), one, 0),
                lambda: ops.displacement_quantiles_update(x, centre, hist, (1.0, 1.0), 0),
                lambda: ops.displacement_quantiles_update(x, centre, hist, (1.0, 0.0, 1.0), 0),
                lambda: ops.displacement_quantiles_update(x, centre, hist, one, -1),
                lambda: ops.displacement_quantiles_update(x, centre, hist, one, 65534),
                lambda: ops.displacement_quantiles_finalize(centre, hist, 0, one, one, pr),
                lambda: ops.displacement_quantiles_finalize(centre, hist, 65536, one, one, pr),
                lambda: ops.displacement_quantiles_finalize(centre.cpu(), hist.cpu(), 2, one, one, pr),
                lambda: ops.displacement_quantiles_finalize(centre.double(), hist, 2, one, one, pr),
                lambda: ops.displacement_quantiles_finalize(centre[0], hist, 2, one, one, pr),
                lambda: ops.displacement_quantiles_finalize(centre, hist[:, :14], 2, one, one, pr),
                lambda: ops.displacement_quantiles_finalize(centre, hist, 2, (1.0, 1.0), one, pr),
                lambda: ops.displacement_quantiles_finalize(centre, hist, 2, one, (1.0, -1.0, 1.0), pr),
                lambda: ops.displacement_quantiles_finalize(centre, hist, 2, one, one, (0.5,)),
                lambda: ops.displacement_quantiles_finalize(centre, hist, 2, one, one, (0.5, 0.4)),
                lambda: ops.displacement_quantiles_finalize(centre, hist, 2, one, one, (0.0, 0.4)),
                lambda: ops.displacement_quantiles_finalize(centre, hist, 2, one, one, [0.1 * k for k in range(1, 10)]),
                lambda: ops.displacement_quantiles_finalize(centre, hist, 2, one, one, pr,
                                                            mask=torch.ones(D, H, W + 1, device=DEV, dtype=torch.bool)),
                lambda: ops.displacement_quantiles_finalize(centre, hist, 2, one, one, pr, mask=torch.ones(D, H, W, device=DEV))):
        with pytest.raises(L.IrsError):
            bad()
    dq = DisplacementQuantiles((D, H, W), DEV, bins=B)
    with pytest.raises(RuntimeError, match='nothing recorded'):
        dq.finalize(PROBS)
    dq.record(x)
    sd = dq.state_dict()
    assert sd['hist'].dtype == torch.uint16 and tuple(sd['hist'].shape) == (3, B, D, H, W) and sd['records'] == 2
    for other in (DisplacementQuantiles((D, H, W + 1), DEV, bins=B), DisplacementQuantiles((D, H, W), DEV, bins=B + 2),
                  DisplacementQuantiles((D, H, W), DEV, bins=B, bin_width=0.25)):
        with pytest.raises(ValueError, match='do not match'):
            other.load_state_dict(sd)
    twin = DisplacementQuantiles((D, H, W), DEV, bins=B)
    twin.load_state_dict(sd)
    assert twin.records == 2 and np.array_equal(hist_np(twin), hist_np(dq)) and torch.equal(twin.centre, dq.centre)


# ---------------------------------------------------------------- the trainer option
def make_trainer(tmp_path, dims, **trainer_over):
    cfg = json.load(open(os.path.join(ROOT, 'configs', 'synthetic_gmm_lognormal.json')))
    cfg['trainer']['save_dir'] = str(tmp_path)
    cfg['data_loader']['args']['dims'] = list(dims)
    cfg['trainer'].update(trainer_over)
    config = ConfigParser.from_dict(copy.deepcopy(cfg), timestamp='t')
    dl = config.init_data_loader()
    losses = config.init_losses()
    tm, rm = config.init_transformation_and_registration_modules()
    return Trainer(config, dl, losses, tm, rm, config.init_metrics(), device=DEV)


NEW_FILES = ['MCMC_disp_ci_width.nii.gz', 'MCMC_disp_ci_width_masked.nii.gz', 'MCMC_disp_q5.vtk', 'MCMC_disp_q50.vtk',
             'MCMC_disp_q95.vtk']


def test_trainer_maps_match_the_recorded_displacements(tmp_path, monkeypatch):
    from ir_sgmcmc_amd.utils.imageio import read_nifti
    N = 24
    import ir_sgmcmc_amd.trainer.trainer as trainer_module
    kept, steps, now = [], [], {}
    record, is_recorded = DisplacementQuantiles.record, trainer_module.is_recorded

    def watch(sample_no, burn_in, period):  # the trainer asks this at every transition: the sample number it is at
        now['sample_no'] = sample_no
        return is_recorded(sample_no, burn_in, period)

    def spy(self, displacement):
        kept.append(displacement.clone())
        steps.append(now['sample_no'])
        return record(self, displacement)

    monkeypatch.setattr(trainer_module, 'is_recorded', watch)
    monkeypatch.setattr(DisplacementQuantiles, 'record', spy)
    kw = dict(no_chains=2, no_iters_burn_in=4, no_samples_MCMC=8, log_period_MCMC=2)
    torch.manual_seed(0)
    # this config's chains wander several voxels between records: 64 bins of 0.75 voxels hold every sample of the run (the
    # default 0.125 leaves half the voxels out of range, which test_trainer_..._resume exercises with the warning)
    wide = 0.75
    t = make_trainer(tmp_path / 'on', (N, N, N), displacement_quantiles={'bin_width': wide}, **kw)
    t.run()
    n = t.no_chains * 4
    assert t.no_chains == 2 and len(kept) == 4 and t._displacement_quantiles.records == n
    assert steps == recorded_steps(4, 8, 2) == [6, 8, 10, 12]  # recorded at these transitions and at no others
    monkeypatch.setattr(DisplacementQuantiles, 'record', record)
    monkeypatch.setattr(trainer_module, 'is_recorded', is_recorded)
    records = torch.cat(kept)  # steps in order, chains in order within a step
    batch = next(iter(t.data_loader))
    mask = batch[1].get('mask', batch[0]['mask']).reshape(N, N, N) != 0
    q, ci, s = calc_displacement_quantiles(records, PROBS, mask.to(DEV), bin_width=wide)
    assert tuple(t.displacement_quantiles.shape) == (3, 3, N, N, N) and tuple(t.displacement_ci_width.shape) == (N, N, N)
    assert torch.equal(t.displacement_quantiles.view(torch.int32), q.view(torch.int32))
    assert torch.equal(t.displacement_ci_width.view(torch.int32), ci.view(torch.int32))
    assert json.dumps(t.displacement_quantiles_summary, sort_keys=True) == json.dumps(s, sort_keys=True)
    dq = t._displacement_quantiles
    check_state(dq, quantiles_np(records.cpu().numpy(), PROBS, bin_width=wide))
    qn, cin = q.cpu().numpy(), ci.cpu().numpy()
    check_outputs(dq, qn, cin, s, PROBS, mask.numpy())
    # everything is in range and within a bin of the order statistic; the median is finite and within the same bound of the
    # sorted records' (no statistical claim about the trainer's mean)
    assert s['out_of_range_voxels'] == 0 and s['clipped_samples'] == 0 and np.isfinite(qn).all() and np.isfinite(cin).all()
    check_bound(records.cpu().numpy(), PROBS, qn, wide, dq.scale)
    assert torch.isfinite(t.displacement_mean).all()
    # files
    folder = t.config.save_dirs['samples']
    plain, _ = read_nifti(str(folder / 'MCMC_disp_ci_width.nii.gz'))
    assert np.array_equal(plain, cin)
    masked, _ = read_nifti(str(folder / 'MCMC_disp_ci_width_masked.nii.gz'))
    m = mask.numpy()
    assert np.array_equal(masked[m], cin[m]) and not masked[~m].any()
    for tag in ('q5', 'q50', 'q95'):
        assert (folder / f'MCMC_disp_{tag}.vtk').stat().st_size > 3 * N ** 3
    # metrics
    res = t.metrics.result()
    for k in QUANTILE_METRICS:
        got, want = res[f'MCMC/quantiles/{k}'], s[k]
        assert (math.isnan(got) and math.isnan(want)) or got == want
    # the same run with the option off: bit-identical chains and displacement moments, and no quantile anything
    torch.manual_seed(0)
    off = make_trainer(tmp_path / 'off', (N, N, N), **kw)
    off.run()
    assert torch.equal(off.v_curr_state, t.v_curr_state)
    assert torch.equal(off.displacement_mean, t.displacement_mean) and torch.equal(off.displacement_std, t.displacement_std)
    assert off.displacement_quantiles is None and off.displacement_ci_width is None and off.displacement_quantiles_summary is None
    assert off._displacement_quantiles is None
    on_keys, off_keys = list(res), list(off.metrics.result())
    assert not [k for k in off_keys if k.startswith('MCMC/quantiles/')]
    assert [k for k in on_keys if not k.startswith('MCMC/quantiles/')] == off_keys
    assert [k for k in on_keys if k.startswith('MCMC/quantiles/')] == [f'MCMC/quantiles/{k}' for k in QUANTILE_METRICS]
    names = lambda tr: sorted(p.name for p in tr.config.save_dirs['samples'].iterdir())
    assert names(t) == sorted(names(off) + NEW_FILES)


def test_trainer_displacement_quantiles_survive_checkpoint_resume_bit_for_bit(tmp_path):
    opt = {'period': 2, 'probs': [0.1, 0.9], 'bins': 32, 'bin_width': 0.25}
    kw = dict(no_chains=2, no_iters_burn_in=2, no_samples_MCMC=8, log_period_MCMC=4, checkpoint_period=6,
              displacement_quantiles=opt, save_outputs=False)
    a = make_trainer(tmp_path / 'a', (16, 16, 16), **kw)
    a.run()
    ck = a.config.save_dirs['checkpoints'] / 'checkpoint_0000006.pt'
    sd = torch.load(ck, map_location='cpu', weights_only=True)
    assert sd['displacement_quantiles']['records'] == 2 * a.no_chains
    assert tuple(sd['displacement_quantiles']['hist'].shape) == (3, 32, 16, 16, 16)
    b = make_trainer(tmp_path / 'b', (16, 16, 16), resume=str(ck), **kw)
    b.run()
    assert a._displacement_quantiles.records == b._displacement_quantiles.records == 8
    # 32 bins of 0.25 voxels are too few for these chains: the out-of-range voxels are NaN, counted, and the same after a resume
    assert a.displacement_quantiles_summary['out_of_range_frac'] > 0 and a.displacement_quantiles.isnan().any()
    assert np.array_equal(hist_np(a._displacement_quantiles), hist_np(b._displacement_quantiles))
    assert torch.equal(a._displacement_quantiles.centre, b._displacement_quantiles.centre)
    assert tuple(a.displacement_quantiles.shape) == (2, 3, 16, 16, 16)
    for name in ('displacement_quantiles', 'displacement_ci_width'):
        assert torch.equal(getattr(a, name).view(torch.int32), getattr(b, name).view(torch.int32)), name
    assert json.dumps(a.displacement_quantiles_summary, sort_keys=True) == json.dumps(b.displacement_quantiles_summary, sort_keys=True)
    # a checkpoint without the key, once a recorded step has passed, is refused
    del sd['displacement_quantiles']
    ck2 = tmp_path / 'no_quantiles.pt'
    torch.save(sd, ck2)
    c = make_trainer(tmp_path / 'c', (16, 16, 16), resume=str(ck2), **kw)
    with pytest.raises(ValueError, match='displacement_quantiles'):
        c.run()
    off_kw = {k: v for k, v in kw.items() if k != 'displacement_quantiles'}
    off = make_trainer(tmp_path / 'off', (16, 16, 16), **off_kw)
    off.run()
    sd_off = torch.load(off.config.save_dirs['checkpoints'] / 'checkpoint_0000006.pt', map_location='cpu', weights_only=True)
    assert set(sd_off) == set(sd)
