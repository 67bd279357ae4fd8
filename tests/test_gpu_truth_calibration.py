"""Known-transformation validation on the GPU: irs_truth_update and irs_truth_calibrate against the float64 restatement
(tests/_truth_calibration.py) -- counts, integer columns, maxima and maps bit for bit, double sums under the bound of a
reordered sum, N * 2^-53 * sum |term| --, the special values, hand-computed dyadic cases, every refusal, truth.known_pair, the
recorder across a restart and the trainer option."""
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
from ir_sgmcmc_amd import truth as T
from ir_sgmcmc_amd.data_loader import synthetic_pair
from ir_sgmcmc_amd.diagnostics import TruthCalibration, recorded_steps
from ir_sgmcmc_amd.parse_config import ConfigParser
from ir_sgmcmc_amd.structure_report import read_csv
from ir_sgmcmc_amd.trainer import Trainer
from ir_sgmcmc_amd.utils import calc_truth_calibration
from tests._truth_calibration import calibrate_np, update_np

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [((5, 6, 7), 1), ((9, 17, 33), 3), ((16, 16, 64), 2)]  # one block; ragged, 20 blocks; 64 blocks
SCALE = (1.5, 0.75, 2.0)
LEVELS = (0.5, 0.9, 0.95)


def dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def to_u16(a):
    return torch.as_tensor(np.ascontiguousarray(a).view(np.int16)).to(DEV).view(torch.uint16)


def from_u16(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def draw(shape, Cn, steps, seed):
    """truth, `steps` records of Cn chains around it (a fifth of the components EQUAL to the truth's), a mask"""
    rng = np.random.default_rng(seed)
    truth = rng.standard_normal((3,) + shape).astype(np.float32)
    u = (truth + 0.7 * rng.standard_normal((steps, Cn, 3) + shape)).astype(np.float32)
    equal = rng.random(u.shape) < 0.2
    u = np.where(equal, truth, u).astype(np.float32)
    mask = rng.random(shape) < 0.6
    return truth, u, mask


def update_sequence(truth, u, mask, scale=SCALE, poison=True):
    below = to_u16(np.full(truth.shape, 0xFFFF if poison else 0, dtype=np.uint16))
    t, m = dev(truth), None if mask is None else dev(mask)
    rows, records = [], 0
    for step in u:
        ints, floats = T.truth_update(dev(step), t, below, records, scale, m)
        rows.append((ints, floats))
        records += step.shape[0]
    torch.cuda.synchronize()
    return from_u16(below), [(i.cpu().numpy(), f.cpu().numpy()) for i, f in rows]


@pytest.mark.parametrize('with_mask', [False, True])
@pytest.mark.parametrize('shape,Cn', CASES)
def test_update_matches_the_restatement(shape, Cn, with_mask):
    truth, u, mask = draw(shape, Cn, 3, 11)
    mask = mask if with_mask else None
    below, rows = update_sequence(truth, u, mask)
    want, records = None, 0
    for step, (ints, floats) in zip(u, rows):
        want, wi, wf, bound = update_np(step, truth, want, records, SCALE, mask)
        records += Cn
        assert np.array_equal(ints, wi)
        assert np.array_equal(floats[:, 2], wf[:, 2])  # the maxima
        err = np.abs(floats[:, :2] - wf[:, :2])
        print({'sum error / bound': (err / bound).max()})
        assert np.all(err <= bound)
    assert np.array_equal(below, want)
    assert below.max() <= 3 * Cn and below.min() == 0
    # the counts do not see the mask; a second identical sequence is bit-identical
    other, rows2 = update_sequence(truth, u, None if with_mask else mask)
    assert np.array_equal(other, below)
    again, rows3 = update_sequence(truth, u, mask)
    assert np.array_equal(again, below)
    for (i1, f1), (i3, f3) in zip(rows, rows3):
        assert np.array_equal(i1, i3) and f1.tobytes() == f3.tobytes()


def test_update_specials():
    shape = (2, 3, 4)
    truth = np.zeros((3,) + shape, dtype=np.float32)
    u = np.zeros((1, 2, 3) + shape, dtype=np.float32)
    u[0, 0, 0, 0, 0, 1] = -1.0      # below; error 1
    u[0, 1, 0, 0, 0, 1] = 1.0       # above
    u[0, 0, 1, 0, 0, 2] = np.nan    # never below, non-finite
    u[0, 1, 1, 0, 0, 2] = -np.inf   # below, non-finite
    u[0, 0, 2, 0, 0, 3] = np.inf    # not below, non-finite
    truth[2, 1, 2, 3] = np.nan      # a NaN truth: nothing is below it, non-finite for both chains
    u[0, :, 2, 1, 2, 3] = -5.0
    u[0, :, 0, 1, 0, 0] = -2.0      # masked out: counted below, not summed
    mask = np.ones(shape, dtype=bool)
    mask[1, 0, 0] = False
    below, rows = update_sequence(truth, u, mask, scale=(1.0, 1.0, 1.0))
    want = np.zeros((3,) + shape, dtype=np.uint16)
    want[0, 0, 0, 1], want[1, 0, 0, 2], want[0, 1, 0, 0] = 1, 1, 2
    assert np.array_equal(below, want)  # u == t exactly is not below
    ints, floats = rows[0]
    assert ints.tolist() == [[23, 3], [23, 2]]
    assert floats.tolist() == [[1.0, 1.0, 1.0], [1.0, 1.0, 1.0]]
    ref = update_np(u[0], truth, None, 0, (1.0, 1.0, 1.0), mask)
    assert np.array_equal(below, ref[0]) and np.array_equal(ints, ref[1]) and np.array_equal(floats, ref[2])
    # an empty mask: zero sums, a maximum nothing entered is -inf
    _, rows = update_sequence(truth, u, np.zeros(shape, dtype=bool))
    assert rows[0][0].tolist() == [[0, 0], [0, 0]] and rows[0][1].tolist() == [[0.0, 0.0, -math.inf]] * 2


def test_update_counts_to_65535_and_refuses_more():
    shape = (2, 2, 3)
    t = torch.zeros((3,) + shape, device=DEV)
    u = torch.full((1, 3) + shape, -1.0, device=DEV)
    below = to_u16(np.full((3,) + shape, 65534, dtype=np.uint16))
    T.truth_update(u, t, below, 65534)
    assert np.all(from_u16(below) == 65535)
    ints = torch.full((1, 2), -5, device=DEV, dtype=torch.int64)
    floats = torch.full((1, 3), -5.0, device=DEV, dtype=torch.float64)
    with pytest.raises(L.IrsError, match='65535'):
        T.truth_update(u, t, below, 65535, out=(ints, floats))
    lib, q = L.load(), lambda x: C.c_void_p(x.data_ptr())
    ws = torch.empty(L.IRS_TRUTH_UPDATE_WS_BYTES, device=DEV, dtype=torch.uint8)
    u2 = torch.full((2, 3) + shape, -1.0, device=DEV)
    with pytest.raises(L.IrsError, match='65534 records \\+ 2 chains'):  # records_before + C = 65536
        L.check(lib.irs_truth_update(q(u2), 2, *shape, q(t), q(below), None, (C.c_float * 3)(1, 1, 1), 65534, q(ints), q(floats), q(ws),
                                     L.IRS_TRUTH_UPDATE_WS_BYTES, L.stream_ptr()))
    torch.cuda.synchronize()
    assert np.all(from_u16(below) == 65535) and bool((ints == -5).all()) and bool((floats == -5.0).all())  # no launch


# ---------------------------------------------------------------- calibrate
def device_state(u):
    """the covariance state and the rank counts of records u (steps,C,3,D,H,W) as the device forms them"""
    shape = u.shape[3:]
    mean = torch.zeros((3,) + shape, device=DEV)
    com = torch.zeros((6,) + shape, device=DEV)
    records = 0
    for step in u:
        ops.displacement_covariance_update(dev(step), mean, com, records)
        records += step.shape[0]
    return mean, com, records


def calibrate_both(mean, com, below, truth, n, mask, scale=SCALE, f=1e-3, rank_bins=16, B=20, R=16, var_edges=None, edges=None,
                   levels=None):
    if edges is None:
        edges, levels = T.calibration_thresholds(n, LEVELS, B, 'hotelling')
    var_edges = T.default_var_edges(R, (0.1, 4.0)) if var_edges is None else var_edges
    got = T.truth_calibrate(mean, com, to_u16(below), dev(truth), n, scale, edges, levels, rank_bins, var_edges, f,
                            None if mask is None else dev(mask))
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in got.items()}
    want = calibrate_np(mean.cpu().numpy(), com.cpu().numpy(), below, truth, n, scale, edges, levels, rank_bins, var_edges, f, mask)
    return got, want


def assert_calibration(got, want):
    for name in ('error', 'mahalanobis'):
        assert np.array_equal(np.isnan(got[name]), np.isnan(want[name])), name
        assert got[name].tobytes() == np.where(np.isnan(want[name]), got[name], want[name]).tobytes(), name  # bit for bit
    for name in ('pit_hist', 'coverage', 'rank_hist', 'isummary'):
        assert np.array_equal(got[name], want[name]), (name, got[name], want[name])
    assert np.array_equal(got['rel_ints'].reshape(-1), want['rel_ints'])
    for j in (2, 4):  # the maxima
        assert got['fsummary'][j] == want['fsummary'][j]
    err = np.abs(got['fsummary'] - want['fsummary'])
    assert np.all(err <= want['fbound']), (err, want['fbound'])
    rel = np.abs(got['rel_floats'] - want['rel_floats'])
    assert np.all(rel <= want['rel_bound']), (rel, want['rel_bound'])
    finite = int(want['isummary'][0] - want['isummary'][1])
    assert got['pit_hist'].sum() == finite and got['rel_ints'].sum() == finite and np.all(got['rank_hist'].sum(axis=1) == finite)


@pytest.mark.parametrize('with_mask', [False, True])
@pytest.mark.parametrize('shape,Cn', CASES)
def test_calibrate_matches_the_restatement(shape, Cn, with_mask):
    truth, u, mask = draw(shape, Cn, 4, 23)
    mask = mask if with_mask else None
    mean, com, n = device_state(u)
    below, _ = update_sequence(truth, u, None)
    # non-finite values in the state and in the truth: NaN in both maps there, counted once
    truth[1].reshape(-1)[3] = np.nan
    mean.view(3, -1)[2, 5] = float('inf')
    com.view(6, -1)[4, 7] = float('nan')
    got, want = calibrate_both(mean, com, below, truth, n, mask)
    assert_calibration(got, want)
    nan_at = np.zeros(shape, dtype=bool)
    nan_at.reshape(-1)[[3, 5, 7]] = True
    assert np.array_equal(np.isnan(got['error']), nan_at) and np.array_equal(np.isnan(got['mahalanobis']), nan_at)
    assert int(want['isummary'][1]) == (3 if mask is None else int(mask.reshape(-1)[[3, 5, 7]].sum()))
    # the maps do not see the mask, and a second call is bit-identical
    other, _ = calibrate_both(mean, com, below, truth, n, None if with_mask else mask)
    again, _ = calibrate_both(mean, com, below, truth, n, mask)
    for name in ('error', 'mahalanobis'):
        assert other[name].tobytes() == got[name].tobytes()
    for name in got:
        assert again[name].tobytes() == got[name].tobytes(), name


def dyadic_state(shape, diag, delta, f):
    """n = 2 records, so that A = comoment + f^2 I: a diagonal power-of-two A and mean - truth = delta, all exact"""
    V = int(np.prod(shape))
    com = np.zeros((6, V), dtype=np.float32)
    for c in range(3):
        com[c] = np.float32(diag[c] - f * f)
        assert float(com[c, 0]) + f * f == diag[c]
    mean = np.tile(np.asarray(delta, dtype=np.float32).reshape(3, 1), (1, V))
    return mean.reshape((3,) + shape), com.reshape((6,) + shape), np.zeros((3,) + shape, dtype=np.float32)


def test_calibrate_dyadic_edges_and_levels():
    """A = diag(4, 16, 1), Delta = (2, 4, 1): d^2 = 1 + 1 + 1 = 3, |Delta|^2 = 21 = tr A.  An edge AT d^2 sends it up a bin; a level
    AT d^2 covers it; an edge at tr A sends it up a reliability bin."""
    shape, f = (2, 2, 4), 2.0 ** -10
    V = 16
    mean, com, truth = dyadic_state(shape, (4.0, 16.0, 1.0), (2.0, 4.0, 1.0), f)
    below = np.zeros((3,) + shape, dtype=np.uint16)
    below[0], below[1], below[2] = 0, 1, 2  # n = 2, B_r = 3: rank r lands in bin r
    just_below = float(np.nextafter(3.0, 0.0))
    got = T.truth_calibrate(dev(mean), dev(com), to_u16(below), dev(truth), 2, (1.0, 1.0, 1.0), [1.0, 3.0, 5.0], [3.0, just_below, 4.0], 3,
                            [8.0, 21.0], f)
    got = {k: v.cpu().numpy() for k, v in got.items()}
    assert got['pit_hist'].tolist() == [0, 0, V, 0]
    assert got['coverage'].tolist() == [V, 0, V]
    assert got['rank_hist'].tolist() == [[V, 0, 0], [0, V, 0], [0, 0, V]]
    assert got['rel_ints'].reshape(-1).tolist() == [0, 0, V] and got['rel_floats'].tolist() == [[0.0, 0.0], [0.0, 0.0], [21.0 * V, 21.0 * V]]
    assert np.all(got['error'] == np.float32(math.sqrt(21.0))) and np.all(got['mahalanobis'] == np.float32(math.sqrt(3.0)))
    assert got['isummary'].tolist() == [V, 0, 0]
    assert got['fsummary'].tolist() == [math.sqrt(21.0) * V, 21.0 * V, math.sqrt(21.0), 3.0 * V, 3.0, 21.0 * V, 1.0 * V, 1.0 * V, 1.0 * V]
    # the scale enters Delta and A alike: d^2 stays 3, the error doubles
    got2 = T.truth_calibrate(dev(mean), dev(com), to_u16(below), dev(truth), 2, (2.0, 2.0, 2.0), [1.0, 3.0, 5.0], [3.0], 3, [], 2.0 ** -9)
    assert got2['pit_hist'].tolist() == [0, 0, V, 0] and bool((got2['error'] == float(2 * np.float32(math.sqrt(21.0)))).all())


def test_calibrate_indefinite_state_is_raised_and_finite():
    shape, f = (2, 3, 4), 1e-3
    V = 24
    mean, com, truth = dyadic_state(shape, (1.0, 1.0, 1.0), (1.0, 1.0, 1.0), 2.0 ** -10)
    com[3] = 5.0  # |xy| > sqrt(xx yy): indefinite; d1 = 1 - 25 < 0
    below = np.zeros((3,) + shape, dtype=np.uint16)
    hand = dict(scale=(1.0, 1.0, 1.0), f=f, rank_bins=4, R=4, edges=[1.0, 2.0, 3.0], levels=[1.0, 5.0])  # (n = 2 has no Hotelling law)
    got, want = calibrate_both(dev(mean), dev(com), below, truth, 2, None, **hand)
    assert_calibration(got, want)
    assert got['isummary'].tolist() == [V, 0, V]
    assert np.isfinite(got['mahalanobis']).all() and np.isfinite(got['fsummary']).all()
    # a negative variance: the first pivot itself
    com[3], com[0] = 0.0, -1.0
    got, want = calibrate_both(dev(mean), dev(com), below, truth, 2, None, **hand)
    assert_calibration(got, want)
    assert got['isummary'].tolist() == [V, 0, V] and np.isfinite(got['fsummary']).all()


def test_abi_and_python_refusals():
    lib = L.load()
    D, H, W, Cn = 4, 5, 6, 2
    f32 = lambda *s: torch.ones(s, device=DEV)
    u, t, mean, com = f32(Cn, 3, D, H, W), f32(3, D, H, W), f32(3, D, H, W), f32(6, D, H, W)
    below = T.new_below((D, H, W), DEV)
    poison_i = lambda *s: torch.full(s, -5, device=DEV, dtype=torch.int64)
    poison_f = lambda *s, dt=torch.float64: torch.full(s, -5.0, device=DEV, dtype=dt)
    ints, floats = poison_i(Cn, 2), poison_f(Cn, 3)
    error, maha = poison_f(D, H, W, dt=torch.float32), poison_f(D, H, W, dt=torch.float32)
    counts, rel_i, rel_f, isum, fsum = poison_i(4 + 2 + 3 * 4), poison_i(3), poison_f(3, 2), poison_i(3), poison_f(9)
    uws = torch.empty(L.IRS_TRUTH_UPDATE_WS_BYTES, device=DEV, dtype=torch.uint8)
    cws = torch.empty(L.IRS_TRUTH_CALIBRATE_WS_BYTES, device=DEV, dtype=torch.uint8)
    q = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    dbl = lambda *v: (C.c_double * max(len(v), 1))(*v)
    flt = lambda *v: (C.c_float * 3)(*v)
    st = L.stream_ptr()

    def update(u_=u, C_=Cn, D_=D, t_=t, below_=below, scale=flt(1, 1, 1), before=0, ints_=ints, floats_=floats, ws_=uws,
               nbytes=L.IRS_TRUTH_UPDATE_WS_BYTES):
        return lib.irs_truth_update(q(u_), C_, D_, H, W, q(t_), q(below_), None, scale, before, q(ints_), q(floats_), q(ws_), nbytes, st)

    def calibrate(mean_=mean, com_=com, below_=below, t_=t, D_=D, n=4, scale=flt(1, 1, 1), f=1e-3, edges=dbl(1.0, 2.0, 3.0), B=4,
                  levels=dbl(1.0, 2.0), Lv=2, Br=4, var=dbl(1.0, 2.0), R=3, error_=error, counts_=counts, ws_=cws,
                  nbytes=L.IRS_TRUTH_CALIBRATE_WS_BYTES):
        return lib.irs_truth_calibrate(q(mean_), q(com_), q(below_), q(t_), D_, H, W, n, scale, f, None, edges, B, levels, Lv, Br, var, R,
                                       q(error_), q(maha), q(counts_), q(rel_i), q(rel_f), q(isum), q(fsum), q(ws_), nbytes, st)

    for kw in (dict(u_=None), dict(t_=None), dict(below_=None), dict(scale=None), dict(ints_=None), dict(floats_=None), dict(ws_=None),
               dict(C_=0), dict(C_=9), dict(D_=1), dict(before=-1), dict(before=65534), dict(scale=flt(1, 0, 1)),
               dict(scale=flt(1, float('nan'), 1)), dict(nbytes=L.IRS_TRUTH_UPDATE_WS_BYTES - 1)):
        with pytest.raises(L.IrsError):
            L.check(update(**kw))
    messages = {}
    for name, kw in (('n=1', dict(n=1)), ('n=65536', dict(n=65536)), ('f=0', dict(f=0.0)), ('f=nan', dict(f=float('nan'))),
                     ('f=inf', dict(f=float('inf'))), ('f=1e-200', dict(f=1e-200)), ('edges', dict(edges=dbl(1.0, 1.0, 3.0))),
                     ('edges nan', dict(edges=dbl(1.0, float('nan'), 3.0))), ('levels inf', dict(levels=dbl(1.0, float('inf')))),
                     ('var', dict(var=dbl(2.0, 1.0))), ('B=0', dict(B=0)), ('B=65', dict(B=65)), ('L=0', dict(Lv=0)), ('L=9', dict(Lv=9)),
                     ('Br=0', dict(Br=0)), ('Br=65', dict(Br=65)), ('R=0', dict(R=0)), ('R=33', dict(R=33)), ('mean', dict(mean_=None)),
                     ('com', dict(com_=None)), ('below', dict(below_=None)), ('truth', dict(t_=None)), ('edges null', dict(edges=None)),
                     ('levels null', dict(levels=None)), ('var null', dict(var=None)), ('error', dict(error_=None)),
                     ('counts', dict(counts_=None)), ('ws', dict(ws_=None)), ('D', dict(D_=1)), ('scale', dict(scale=flt(-1, 1, 1))),
                     ('bytes', dict(nbytes=L.IRS_TRUTH_CALIBRATE_WS_BYTES - 1))):
        with pytest.raises(L.IrsError) as info:
            L.check(calibrate(**kw))
        messages[name] = str(info.value)
    # the refusal names the value
    for name, word in (('n=1', 'n = 1'), ('n=65536', '65536'), ('f=0', 'std_floor = 0'), ('f=1e-200', '1e-200'), ('edges', 'd2_edges[1] = 1'),
                       ('var', 'var_edges[1] = 1'), ('B=65', 'pit_bins = 65'), ('L=9', 'n_levels = 9'), ('Br=0', 'rank_bins = 0'),
                       ('R=33', 'reliability_bins = 33'), ('levels inf', 'levels[1] = inf')):
        assert word in messages[name], (name, messages[name])
    torch.cuda.synchronize()
    for x in (ints, floats, error, maha, counts, rel_i, rel_f, isum, fsum):  # a refused call writes nothing
        assert bool((x == -5).all())
    assert int(from_u16(below).max()) == 0
    L.check(update())
    L.check(calibrate())
    L.check(calibrate(B=1, edges=None, R=1, var=None))  # one bin needs no edge
    torch.cuda.synchronize()
    assert ints.tolist() == [[D * H * W, 0]] * Cn and isum.tolist() == [D * H * W, 0, 0] and int(counts[0]) == D * H * W
    # the Python surface checks dtypes, shapes and devices before it calls
    edges, levels, var = [1.0, 2.0], [1.0], [1.0]
    for bad in (lambda: T.truth_update(u.double(), t, below, 0), lambda: T.truth_update(u, t.double(), below, 0),
                lambda: T.truth_update(u, t, below.view(torch.int16), 0), lambda: T.truth_update(u, t[:, :2].contiguous(), below, 0),
                lambda: T.truth_update(u.cpu(), t.cpu(), below.cpu(), 0), lambda: T.truth_update(u, t, below, -1),
                lambda: T.truth_update(u, t, below, 0, scale=(1.0, 2.0)), lambda: T.truth_update(u, t, below, 0, scale=(1.0, -2.0, 1.0)),
                lambda: T.truth_update(u, t, below, 0, mask=torch.ones(D, H, W, device=DEV)),
                lambda: T.truth_update(u, t, below, 0, out=(ints.int(), floats)), lambda: T.truth_update(u, t, below, 0, out=(ints, floats[:, :2])),
                lambda: T.truth_calibrate(mean.double(), com, below, t, 4, (1, 1, 1), edges, levels, 4, var),
                lambda: T.truth_calibrate(mean, com[:5].contiguous(), below, t, 4, (1, 1, 1), edges, levels, 4, var),
                lambda: T.truth_calibrate(mean, com, below, t, 1, (1, 1, 1), edges, levels, 4, var),
                lambda: T.truth_calibrate(mean, com, below, t, 4.5, (1, 1, 1), edges, levels, 4, var),
                lambda: T.truth_calibrate(mean, com, below, t, 4, (1, 1, 1), [2.0, 1.0], levels, 4, var),
                lambda: T.truth_calibrate(mean, com, below, t, 4, (1, 1, 1), edges, [], 4, var),
                lambda: T.truth_calibrate(mean, com, below, t, 4, (1, 1, 1), edges, levels, 65, var),
                lambda: T.truth_calibrate(mean, com, below, t, 4, (1, 1, 1), edges, levels, 4, var, std_floor=-1.0),
                lambda: T.truth_calibrate(mean, com, below, t, 4, (1, 1, 1), edges, levels, 4, var, std_floor='small'),
                lambda: T.truth_calibrate(mean.cpu(), com.cpu(), below.cpu(), t.cpu(), 4, (1, 1, 1), edges, levels, 4, var)):
        with pytest.raises(L.IrsError):
            bad()


@pytest.mark.parametrize('shape', [(41, 40, 41), (65, 64, 65)])
def test_both_kernels_past_one_round_of_either_stage(shape):
    """(41,40,41): 257 blocks of partials against the 256 threads that fold them; (65,64,65): 270 400 voxels against the 1024 x
    256 a grid covers in one round"""
    truth, u, mask = draw(shape, 1, 4, 5)
    below, rows = update_sequence(truth, u, mask)
    want, records = None, 0
    for step, (ints, floats) in zip(u, rows):
        want, wi, wf, bound = update_np(step, truth, want, records, SCALE, mask)
        records += 1
        assert np.array_equal(ints, wi) and np.array_equal(floats[:, 2], wf[:, 2])
        assert np.all(np.abs(floats[:, :2] - wf[:, :2]) <= bound)
    assert np.array_equal(below, want)
    mean, com, n = device_state(u)
    got, want = calibrate_both(mean, com, below, truth, n, mask)
    assert_calibration(got, want)


# ---------------------------------------------------------------- the pair with a known transformation
def fixed_triple(dims, noise=0.02):
    f, _ = synthetic_pair(dims, seed=0, noise=noise)
    return {k: v.unsqueeze(0).to(DEV) for k, v in f.items()}


def test_known_pair_of_a_zero_velocity_is_the_fixed_triple():
    dims = (8, 9, 10)
    fixed = fixed_triple(dims)
    moving, truth, info = T.known_pair(fixed, T.simulate_velocity(dims, 0, 0.0), 12)
    for key in ('im', 'mask', 'seg'):
        assert moving[key].dtype == fixed[key].dtype and torch.equal(moving[key], fixed[key]) and moving[key] is not fixed[key]
    assert not bool(truth.any()) and info['amplitude'] == 0.0 and info['floor_max'] == 0.0 and info['floor_mean'] == 0.0
    noisy, _, _ = T.known_pair(fixed, np.zeros((3,) + dims, dtype=np.float32), 12, noise=0.05, seed=3)
    again, _, _ = T.known_pair(fixed, np.zeros((3,) + dims, dtype=np.float32), 12, noise=0.05, seed=3)
    assert torch.equal(noisy['im'], again['im']) and torch.equal(noisy['mask'], fixed['mask'])
    assert float((noisy['im'] - fixed['im']).std()) == pytest.approx(0.05, rel=0.1)


def test_known_pair_truth_and_error_floor():
    """(16, 20, 24), amplitude 2, seed 0, 12 steps: the CPU oracle's construction (oracle.ops.svf_exp of v and of -v, composed by
    grid_sample) has |phi*^-1 o phi* - id| of mean 0.0678 and max 0.322 voxels over the 2944 voxels of the fixed mask; the device
    sums in another order and its gathers round differently, so the floor is held to twice those values."""
    dims, steps = (16, 20, 24), 12
    fixed = fixed_triple(dims, noise=0.0)
    v = T.simulate_velocity(dims, 0, 2.0)
    moving, truth, info = T.known_pair(fixed, v, steps)
    vd = dev(v).unsqueeze(0)
    t_fwd, d_fwd, _ = ops.svf_exp_fwd(vd, steps)
    t_inv, d_inv = ops.svf_exp_inverse(vd, steps)
    assert torch.equal(truth, d_fwd[0]) and info['amplitude'] == 2.0 and info['truth_max'] == float(d_fwd.abs().max())
    _, _, isum, fsum = ops.inverse_consistency(t_fwd, d_fwd, d_inv, mask=fixed['mask'])
    voxels = int(isum[0, 0] - isum[0, 1])
    assert voxels == info['floor_voxels'] == 2944
    assert info['floor_mean'] == float(fsum[0, 0]) / voxels and info['floor_max'] == float(fsum[0, 2])
    print(info)
    assert 0 < info['floor_mean'] <= 2 * 0.0678 and info['floor_max'] <= 2 * 0.322
    # the moving triple is the fixed one through the inverse map, so the truth brings it back
    assert torch.equal(moving['im'], ops.warp(fixed['im'], t_inv)) and torch.equal(moving['seg'], ops.warp(fixed['seg'], t_inv))
    assert moving['mask'].dtype == torch.bool and moving['seg'].dtype == torch.int16
    back = ops.warp(moving['im'], t_fwd)
    m = fixed['mask']
    before, after = float((moving['im'] - fixed['im'])[m].abs().mean()), float((back - fixed['im'])[m].abs().mean())
    print({'mean |moving - fixed|': before, 'mean |moving o phi* - fixed|': after})
    assert after < 0.5 * before
    with pytest.raises(L.IrsError, match='v_true'):
        T.known_pair(fixed, v[:, :8], steps)
    with pytest.raises(L.IrsError, match='noise'):
        T.known_pair(fixed, v, steps, noise=-1.0)


# ---------------------------------------------------------------- the recorder
def test_recorder_survives_a_restart_and_equals_the_functional_form():
    shape, Cn, steps = (9, 17, 33), 2, 5
    truth, u, mask = draw(shape, Cn, steps, 31)
    kw = dict(levels=LEVELS, pit_bins=10, rank_bins=5, reliability_bins=8, std_floor=1e-3, reference='hotelling')
    whole = TruthCalibration(dev(truth), steps * Cn, DEV, SCALE, dev(mask))
    for step in u:
        whole.record(dev(step))
    maps, s, (ints, floats) = whole.finalize(**kw, initial=whole.initial_error())
    first = TruthCalibration(dev(truth), steps * Cn, DEV, SCALE, dev(mask))
    for step in u[:2]:
        first.record(dev(step))
    sd = first.state_dict()
    assert sd['records'] == 4 and sd['fingerprint'] == T.fingerprint(truth) and sd['covariance']['records'] == 4
    second = TruthCalibration(dev(truth), steps * Cn, DEV, SCALE, dev(mask))
    second.load_state_dict(sd)
    for step in u[2:]:
        second.record(dev(step))
    maps2, s2, (ints2, floats2) = second.finalize(**kw, initial=second.initial_error())
    assert torch.equal(maps['error'], maps2['error']) and torch.equal(maps['mahalanobis'], maps2['mahalanobis'])
    assert json.dumps(s, sort_keys=True) == json.dumps(s2, sort_keys=True)
    assert np.array_equal(ints, ints2) and floats.tobytes() == floats2.tobytes()
    # the series rows are the update's own, and the initial error is the update on a zero displacement
    _, rows = update_sequence(truth, u, mask, poison=False)
    assert np.array_equal(ints, np.concatenate([r[0] for r in rows])) and np.array_equal(floats, np.concatenate([r[1] for r in rows]))
    _, zi, zf, _ = update_np(np.zeros((1, 3) + shape, dtype=np.float32), truth, None, 0, SCALE, mask)
    assert s['initial_rmse'] == pytest.approx(math.sqrt(zf[0, 1] / zi[0, 0]), rel=1e-12) and s['initial_max'] == zf[0, 2]
    # against the restatement of the whole, and the one-call form
    mean, com, n = device_state(u)
    below, _ = update_sequence(truth, u, None)
    edges, lv = T.calibration_thresholds(n, LEVELS, 10)
    want = calibrate_np(mean.cpu().numpy(), com.cpu().numpy(), below, truth, n, SCALE, edges, lv, 5, T.default_var_edges(8), 1e-3, mask)
    assert s['pit_hist'] == want['pit_hist'].tolist() and s['rank_hist'] == want['rank_hist'].tolist()
    assert [row['count'] for row in s['coverage'].values()] == want['coverage'].tolist()
    assert np.array_equal(np.isnan(maps['error'].cpu().numpy()), np.isnan(want['error']))
    assert maps['error'].cpu().numpy().tobytes() == want['error'].tobytes()
    maps3, s3, _ = calc_truth_calibration(dev(u.reshape((-1, 3) + shape)), dev(truth), dev(mask), Cn, SCALE, **kw)
    assert torch.equal(maps3['mahalanobis'], maps['mahalanobis']) and json.dumps(s3, sort_keys=True) == json.dumps(s, sort_keys=True)
    # another truth, another shape, too many records
    other = TruthCalibration(dev(truth + 1), steps * Cn, DEV, SCALE, dev(mask))
    with pytest.raises(ValueError, match='another truth'):
        other.load_state_dict(sd)
    small = TruthCalibration(dev(truth), 2, DEV, SCALE, dev(mask))
    with pytest.raises(ValueError, match='does not match'):
        small.load_state_dict(sd)
    small.record(dev(u[0]))
    with pytest.raises(ValueError, match='2 rows'):
        small.record(dev(u[1]))
    with pytest.raises(RuntimeError, match='at least 6'):
        small.finalize()


# ---------------------------------------------------------------- the trainer option
TRUTH = {'source': 'simulate', 'amplitude': 2.0, 'seed': 0, 'period': 2, 'rank_bins': 8}
RUN = dict(no_chains=2, no_iters_burn_in=150, no_samples_MCMC=60, log_period_MCMC=30)


def make_trainer(tmp_path, dims, **trainer_over):
    cfg = json.load(open(os.path.join(ROOT, 'configs', 'synthetic_ssd_l2_128.json')))
    cfg['trainer']['save_dir'] = str(tmp_path)
    cfg['data_loader']['args']['dims'] = list(dims)
    cfg['trainer'].update(trainer_over)
    config = ConfigParser.from_dict(copy.deepcopy(cfg), timestamp='t')
    dl = config.init_data_loader()
    losses = config.init_losses()
    tm, rm = config.init_transformation_and_registration_modules()
    return Trainer(config, dl, losses, tm, rm, config.init_metrics(), device=DEV)


def test_trainer_end_to_end(tmp_path):
    N = 32
    t = make_trainer(tmp_path / 'on', (N, N, N), truth=TRUTH, **RUN)
    t.run()
    s, tc = t.truth_summary, t._truth_calibration
    steps = recorded_steps(RUN['no_iters_burn_in'], RUN['no_samples_MCMC'], 2)
    assert len(steps) == 30 and tc.records == s['records'] == 60
    fixed_mask = next(iter(t.data_loader))[0]['mask'].reshape(N, N, N)
    V = int(fixed_mask.sum())
    assert s['voxels'] == V and s['nonfinite_voxels'] == 0
    # the registration brings the posterior mean closer to the truth than the identity is
    print({k: s[k] for k in ('rmse', 'mean', 'max', 'initial_rmse', 'initial_mean', 'initial_max', 'scale_factor', 'ence', 'floor_mean',
                             'floor_max')}, {k: v['observed'] for k, v in s['coverage'].items()})
    assert 0 < s['rmse'] < s['initial_rmse'] and s['initial_max'] <= math.sqrt(3) * float(t._truth.abs().max()) + 1e-6
    assert 0 < s['floor_mean'] <= s['floor_max']
    assert sum(sum(h) for h in s['rank_hist']) == 3 * V and sum(s['pit_hist']) == V
    assert sum(r['count'] for r in s['reliability']) == V
    assert list(s['coverage']) == ['50', '90', '95'] and all(0 <= r['observed'] <= 1 for r in s['coverage'].values())
    assert s['coverage']['50']['count'] <= s['coverage']['90']['count'] <= s['coverage']['95']['count']
    # metrics
    res = t.metrics.result()
    for key in T.METRIC_KEYS:
        assert res[f'MCMC/truth/{key}'] == s[key], key
    for key, row in s['coverage'].items():
        assert res[f'MCMC/truth/coverage_{key}'] == row['observed']
    for key in T.INITIAL_METRICS:
        assert res[f'truth/initial/{key}'] == s[f'initial_{key}']
    # files
    folder = t.config.save_dirs['samples']
    names = sorted(p.name for p in folder.iterdir())
    for name in ('MCMC_truth_error.nii.gz', 'MCMC_truth_error_masked.nii.gz', 'MCMC_truth_mahalanobis.nii.gz',
                 'MCMC_truth_mahalanobis_masked.nii.gz', 'MCMC_truth_calibration.csv', 'MCMC_truth_series.csv', 'truth_displacement.vtk'):
        assert name in names, names
    header, rows = read_csv(folder / 'MCMC_truth_calibration.csv')
    assert header == ['table', 'bin', 'count', 'expected', 'lo', 'hi', 'value_a', 'value_b']
    tables = [r[0] for r in rows]
    assert [tables.count(k) for k in ('pit', 'rank_x', 'rank_y', 'rank_z', 'reliability', 'coverage')] == [20, 8, 8, 8, 16, 3]
    assert [r[2] for r in rows if r[0] == 'pit'] == s['pit_hist'] and [r[2] for r in rows if r[0] == 'rank_y'] == s['rank_hist'][1]
    assert [r[3] for r in rows if r[0] == 'rank_z'] == s['rank_expected']
    sheader, srows = read_csv(folder / 'MCMC_truth_series.csv')
    assert tuple(sheader) == T.SERIES_COLUMNS and len(srows) == 60
    assert [r[1] for r in srows] == [st for st in steps for _ in range(2)] and [r[2] for r in srows] == [0, 1] * 30
    assert all(r[6] == V and r[7] == 0 and 0 < r[3] <= r[4] <= r[5] for r in srows)
    # the saved truth reads back as the truth (the synthetic pair has unit spacing)
    back = T.read_truth(folder / 'truth_displacement.vtk', (N, N, N), 'mm')
    assert np.array_equal(back, t._truth.cpu().numpy())
    # the error map is the distance of the posterior mean from the truth
    err = (t._truth_calibration.covariance.mean - t._truth).double().pow(2).sum(0).sqrt()
    assert float((t.truth_error.double() - err).abs().max()) < 1e-6


def test_trainer_checkpoint_resume_is_bit_identical(tmp_path):
    kw = dict(no_chains=2, no_iters_burn_in=4, no_samples_MCMC=12, log_period_MCMC=6, checkpoint_period=10,
              truth={**TRUTH, 'reference': 'chi2'})
    a = make_trainer(tmp_path / 'a', (16, 16, 16), **kw)
    a.run()
    ck = a.config.save_dirs['checkpoints'] / 'checkpoint_0000010.pt'
    sd = torch.load(ck, map_location='cpu', weights_only=True)
    assert sd['truth_calibration']['records'] == 6 and tuple(sd['truth_calibration']['below'].shape) == (3, 16, 16, 16)
    b = make_trainer(tmp_path / 'b', (16, 16, 16), resume=str(ck), **kw)
    b.run()
    assert json.dumps(a.truth_summary, sort_keys=True) == json.dumps(b.truth_summary, sort_keys=True)
    assert torch.equal(a.truth_error, b.truth_error) and torch.equal(a.truth_mahalanobis, b.truth_mahalanobis)
    for name in ('MCMC_truth_calibration.csv', 'MCMC_truth_series.csv'):
        fa, fb = (x.config.save_dirs['samples'] / name for x in (a, b))
        assert fa.read_bytes() == fb.read_bytes() and fa.stat().st_size > 0, name
    # a resume on another truth is refused
    c = make_trainer(tmp_path / 'c', (16, 16, 16), resume=str(ck), **{**kw, 'truth': {**kw['truth'], 'seed': 1}})
    with pytest.raises(ValueError, match='another truth'):
        c.run()


def test_trainer_refusals_and_a_run_without_the_option(tmp_path):
    with pytest.raises(ValueError, match='affine_init'):
        make_trainer(tmp_path / 'x', (16, 16, 16), truth=TRUTH, affine_init={'model': 'rigid'}, **RUN)
    with pytest.raises(ValueError, match='landmarks'):
        make_trainer(tmp_path / 'y', (16, 16, 16), truth=TRUTH, landmarks={'synthetic': True}, **RUN)
    with pytest.raises(ValueError, match="'colour'"):
        make_trainer(tmp_path / 'z', (16, 16, 16), truth={**TRUTH, 'colour': 1}, **RUN)
    off = make_trainer(tmp_path / 'off', (16, 16, 16), no_chains=2, no_iters_burn_in=2, no_samples_MCMC=6, log_period_MCMC=3,
                       checkpoint_period=4)
    off.run()
    assert off.truth_summary is None and off._truth is None and off._truth_calibration is None
    assert not [k for k in off.metrics.result() if 'truth' in k]
    sd = torch.load(off.config.save_dirs['checkpoints'] / 'checkpoint_0000004.pt', map_location='cpu', weights_only=True)
    assert 'truth_calibration' not in sd
    assert not [p.name for p in off.config.save_dirs['samples'].iterdir() if 'truth' in p.name]
