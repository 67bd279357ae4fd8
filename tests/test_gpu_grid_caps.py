"""Every capped launch past its block cap, against the float64 restatement its family already has.

Each reduction and streaming kernel outside the transition launches min(ceil(units / 256), cap) blocks; at the volumes the
project runs on every one of them is capped, its threads make several trips and the second stage folds several rows of
partials per thread.  tests/_grid_caps.py holds the table of those launches and, per record, the smallest convenient ragged
shape past the cap; tests/test_grid_caps_host.py checks the caps against the source and proves that the inputs used here tell a
dropped tail, a tail counted twice and a second stage that stops after one round from the right answer.  Here the public
operators run on those inputs.  Per-voxel outputs are compared element by element under the tolerance rule of the family's own
GPU test (the line is named at each use), integer outputs for equality, float summary columns against the restatement of the
maps the device stored.  Every comparison goes through tests/_report.check.

Pre-filling.  The states the callers own are filled with NaN or a sentinel wherever the operator's contract lets it overwrite
them (the updates with records_before = 0, the Gram matrix): there an element that was not visited is certain to show.  The
outputs the wrappers allocate themselves cannot be filled from outside.  `poison` leaves blocks of NaN (or -7) of the same
sizes with the caching allocator just before the call and reports whether a probe allocation got them back; that is no
guarantee -- the allocator may round, split or order its blocks otherwise -- and no assertion rests on it.  What those outputs
rest on is the element-by-element comparison itself: an element that was not written holds whatever the block held before,
which would have to agree with the reference within the tolerance to go unnoticed.

The chosen shapes (record: shape, chains -> blocks x trips; the corrections to the issue's table are marked *):
  modes_gram_partial_kernel                  (41,41,41)     256 x 2   (68 921 voxels, odd; n_before 2 + 3 new records)
  precond_mean_kernel<0/1>, precond_field_kernel and the two finish kernels
                                             (45,45,45)    1024 x 2   (N = 3 V = 273 375)
  chain_moments_kernel<VEC>                  (71,71,72) C2 2048 x 2  *(units of four over the C 3 V elements of a half: it wraps
                                                                      past C 3 V / 4 = 524 288; both halves aligned here)
  chain_moments_kernel<scalar>               (57,57,57) C1 2048 x 2  *(the form is picked by pointer alignment alone and half 1
                                                                      starts C 3 V floats into the state: with C 3 V = 555 579, odd,
                                                                      its four updates are scalar; half 0 is vector with a tail)
  split_rhat_kernel, split_ess_kernel        (89,88,90) C2 2048 x 2
  chain_variogram_kernel<VEC>                (89,88,90) C2 2048 x 2   (E = 3 V elements, the chains inside the loop)
  chain_variogram_kernel<scalar>             (57,57,57) C1 2048 x 2   (E = 555 579, odd)
  inverse_consistency_kernel                 (65,65,65) C2 1024 x 2 per chain
  inverse_consistency_update_kernel          (101,102,103) C2 4096 x 2
  negate_kernel                              (71,71,71) C1 4096 x 2  *(it streams C 3 V elements: past 349 525 voxels at C = 1)
  inverse_consistency_finalize_kernel        (65,65,65)    1024 x 2
  local_similarity_kernel<1>                 (1361,17,33) C2: 6 tiles x 171 segments = 1026 work items on 1024 blocks
                                                                     *(763 521 voxels: the smallest volume whose tile count
                                                                      does not divide 1024 and whose depth allows the segments)
  local_similarity_update_kernel             (101,102,103) C2 4096 x 2
  local_similarity_finalize_kernel           (65,65,65)    1024 x 2
  residual_histogram_kernel<scalar>          (65,65,65) C2 1024 x 2 per chain
  residual_histogram_kernel<VEC>             (101,102,104) C2 1024 x 2 per chain
  residual_nll_update_kernel                 (101,102,103) C2 4096 x 2
  residual_nll_finalize_kernel               (65,65,65)    1024 x 2
  similarity_accumulate_kernel<scalar> C=8   (33,33,33)     128 x 2 per chain
  similarity_accumulate_kernel<VEC> C=8      (52,51,52)     128 x 2 per chain
  similarity_accumulate_kernel<scalar> C=1   (65,65,65)    1024 x 2
  similarity_accumulate_kernel<VEC> C=1      (101,102,104) 1024 x 2
  label_update_kernel<scalar>                (65,65,65) C2 1024 x 2
  label_update_kernel<VEC>                   (130,127,128) C2 1024 x 2 *(units of 8 voxels: the cap is passed above 2 097 152 voxels,
                                                                      not at 262 144; the existing 64^3 case is the scalar cap exactly)
  label_finalize_kernel                      (65,65,65)    1024 x 2
  surface_finalize_kernel                    (47,45,9)      512 x 2   (2115 rows, 4 per block)
  intensity_histogram_kernel                 (65,65,65) C2 1024 x 2 per volume
  cc_scan_kernel                             (101,102,103) C2: 1037 chunks, 2 per thread
  select_largest_kernel                      (101,102,103) C2: 1157 components, a second sweep trip of the 1024 threads
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from ir_sgmcmc_amd import _lib as L
from ir_sgmcmc_amd import masks as M
from ir_sgmcmc_amd import modes, ops
from ir_sgmcmc_amd import preconditioner as P
from ir_sgmcmc_amd import residual_check as RC
from ir_sgmcmc_amd.diagnostics import ChainMoments
from tests import _grid_caps as G
from tests._report import check

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U = 2.0 ** -24


def dev(a):
    if a is None:
        return None
    return (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(DEV).contiguous()


def poison(*specs):
    """blocks of NaN (floating point) or -7 (integers) of the given (shape, dtype), handed back to the caching allocator, which
    usually returns them to the next torch.empty of those sizes -> whether a probe allocation saw every fill (best effort:
    see the module docstring)"""
    fill = lambda dtype: float('nan') if dtype.is_floating_point else -7
    held_ = [torch.full(tuple(shape), fill(dtype), device=DEV, dtype=dtype) for shape, dtype in specs]
    torch.cuda.synchronize()
    del held_
    probes = [torch.empty(tuple(shape), device=DEV, dtype=dtype) for shape, dtype in specs]  # what the wrapper is about to get
    back = [bool(torch.isnan(p).all()) if p.dtype.is_floating_point else bool((p == -7).all()) for p in probes]
    print(f'poison: {sum(back)} of {len(back)} blocks came back filled')
    del probes
    return all(back)


def used(err, tol):
    """the fraction of the tolerance a deviation uses, elementwise; a deviation where the tolerance is 0 is infinite"""
    err = np.asarray(err, np.float64)
    tol = np.broadcast_to(np.asarray(tol, np.float64), err.shape)
    return np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err > 0, np.inf, 0.0))


def held(test, key, got, ref, tol):
    """|got - ref| <= tol wherever ref is finite; NaN exactly where ref is NaN, and the same infinity where it is infinite"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (test, key, got.shape, ref.shape)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (test, key, int(np.isnan(got).sum()), int(np.isnan(ref).sum()))
    assert np.array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)]), (test, key, 'infinities')
    tol = np.broadcast_to(np.asarray(tol, np.float64), ref.shape)
    u = used(np.abs(got[fin] - ref[fin]), tol[fin])
    worst = check(test, key + ' / tolerance', u, np.zeros_like(u), 1.0)
    print(f'{test}: {key}: worst deviation / tolerance {worst:.3g}')
    return worst


def same(test, key, got, ref):
    """integers: equal"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (test, key, got.shape, ref.shape)
    check(test, key, got.astype(np.int64), ref.astype(np.int64), 0)


def T(name):
    return f'grid_caps/{name}'


def geometry_line(name):
    rec = G.RECORD[name]
    g = G.geometry(rec)
    print(f'{name}: shape {rec.shape} chains {rec.chains}: {g.units} units, {g.blocks} blocks x {g.trips} trips')
    assert g.trips >= 2
    return rec, g


# ---------------------------------------------------------------- modes
@pytest.mark.parametrize('name', G.records_of('modes'))
def test_modes(name):
    from tests import _displacement_modes as R
    rec, g = geometry_line(name)
    case = G.case('modes/gram')
    nbytes = C.c_size_t()  # the chunks the library itself counts (irs_modes_gram_workspace: chunks x n_new x 3 x 1024 doubles)
    L.check(L.load().irs_modes_gram_workspace(*rec.shape, 3, C.byref(nbytes)))
    assert nbytes.value == g.blocks * 3 * 3 * L.IRS_MODES_MAX_RECORDS * 8
    n = sum(case['appends'])
    for masked in (True, False):
        records = case['spoiled'] if masked else case['records']
        st = modes.modes_state(rec.shape, n, DEV, dev(case['mask']) if masked else None)
        st['gram'].fill_(float('nan'))
        x, at = dev(records), 0
        for c in case['appends']:  # n_before = 0 with two new records, then n_before = 2 with an odd three
            modes.modes_append(st, x[at:at + c].contiguous())
            at += c
        Gm = modes.modes_gram(st)
        ref, bound = case['gram'][masked]
        assert np.array_equal(Gm, np.transpose(Gm, (0, 2, 1)))
        held(T(name), f'gram, mask {masked}', Gm, ref, bound)  # tests/test_gpu_displacement_modes.py:58-65
    # the projection at the same V, on the state without a mask: mean and modes bit for bit, the explained ratio in its bound
    coeff = np.random.default_rng(3).standard_normal((3, n))
    scale = R.default_scale(rec.shape)
    poison(((3, *rec.shape), torch.float32), ((3, 3, *rec.shape), torch.float32), (rec.shape, torch.float32))
    mean, fields, explained = modes.modes_project(st, coeff, scale)
    want = R.project_np(case['records'], coeff, scale)
    held(T(name), 'projected mean', mean.cpu().numpy(), want['mean'], 0)       # tests/test_gpu_displacement_modes.py:124-125
    held(T(name), 'projected modes', fields.cpu().numpy(), want['modes'], 0)
    e, B, ok = R.explained_ref(case['records'], coeff, scale)
    assert ok.all()
    held(T(name), 'explained', explained.cpu().numpy(), e, B)                    # tests/_displacement_modes.py:305-317


# ---------------------------------------------------------------- preconditioner
@functools.lru_cache(maxsize=None)
def precond_run(smooth):
    from tests import _preconditioner as S
    case = G.case(f'preconditioner/smooth{smooth}')
    rec = case['record']
    o = G.PRECOND
    state = P.preconditioner_state(rec.shape, DEV)
    state['V'].copy_(dev(case['V']))
    state['count'] = o['count']
    Cn = 2
    poison(((Cn, 3, *rec.shape), torch.float32), ((L.IRS_PRECOND_SUMMARY,), torch.float64))
    sigma, got = P.preconditioner_sigma(state, Cn, o['beta'], smooth=smooth, damping=o['damping'], sigma_min=o['sigma_min'],
                                        sigma_max=o['sigma_max'])
    V = case['V']
    bias = S.bias_correction(o['beta'], o['count'])
    sbar, _ = S.means(V, bias, smooth, o['damping'])
    _, gbar = S.means(V, bias, smooth, o['damping'], sbar=got['s_mean'])
    want, summary = S.sigma_field(V, Cn, bias, smooth, o['damping'], o['sigma_min'], o['sigma_max'], sbar=got['s_mean'], gbar=got['G_mean'])
    return {'sigma': sigma.cpu().numpy(), 'got': got, 'sbar': sbar, 'gbar': gbar, 'want': want, 'summary': summary, 'N': V.size}


@pytest.mark.parametrize('smooth', [0, 1])
@pytest.mark.parametrize('name', G.records_of('preconditioner'))
def test_preconditioner(name, smooth):
    geometry_line(name)
    r = precond_run(smooth)
    got, summary, rel = r['got'], r['summary'], r['N'] * 2.0 ** -52  # tests/test_gpu_preconditioner.py:101-108
    t = T(f'{name} smooth {smooth}')
    # one run per smooth value; every record holds the part of it that its kernel produces
    if name.endswith('precond_mean_kernel<0>'):        # the partial sums of s
        held(t, 's_mean', got['s_mean'], r['sbar'], rel * r['sbar'])
    elif name.endswith('precond_mean_kernel<1>'):      # the partial sums of G, formed with the device's own mean of s
        held(t, 'G_mean', got['G_mean'], r['gbar'], rel * r['gbar'])
    elif name.endswith('precond_mean_finish_kernel'):  # the second stage of both: four rows of partials per thread
        held(t, 's_mean', got['s_mean'], r['sbar'], rel * r['sbar'])
        held(t, 'G_mean', got['G_mean'], r['gbar'], rel * r['gbar'])
    elif name.endswith('precond_field_kernel'):        # the field, bit for bit with the device's own means, every chain's copy
        held(t, 'sigma', r['sigma'], r['want'], 0)
    else:                                              # the summary: the rows of the field kernel's partials folded
        for key_ in ('clamped_low', 'clamped_high', 'nonfinite'):
            same(t, key_, got[key_], summary[key_])
        held(t, 'sigma_min', got['sigma_min'], summary['sigma_min'], 0)
        held(t, 'sigma_max', got['sigma_max'], summary['sigma_max'], 0)
        held(t, 'sigma2_mean', got['sigma2_mean'], summary['sigma2_mean'], rel * summary['sigma2_mean'])
        assert got['clamped_low'] > 0 and got['clamped_high'] > 0


# ---------------------------------------------------------------- chain diagnostics
def moments_np(x):
    """tests/test_gpu_chain_diagnostics.py:42-49: per-half, per-chain mean and M2 in float64 -> (2, C, 3, V) each"""
    n = x.shape[1] // 2
    with np.errstate(all='ignore'):
        halves = [x[:, :n].astype(np.float64), x[:, x.shape[1] - n:].astype(np.float64)]
        mean = np.stack([h.mean(axis=1) for h in halves])
        m2 = np.stack([((h - h.mean(axis=1, keepdims=True)) ** 2).sum(axis=1) for h in halves])
    return mean, m2


def record_chain(x, shape):
    cm = ChainMoments(x.shape[0], shape, x.shape[1], DEV, max_lag=G.DIAG_LAG)
    xd = dev(x.reshape(*x.shape[:3], *shape))
    for i in range(x.shape[1]):  # eight folds: k = 1 and then k > 1 of both halves
        cm.record(xd[:, i].contiguous())
    return cm


@functools.lru_cache(maxsize=None)
def diag_run():
    case = G.case('diagnostics/finalize')
    shape = case['record'].shape
    cm = record_chain(case['x'], shape)
    mask = dev(case['mask'])
    poison((shape, torch.float32), ((5,), torch.float64))
    rhat, rsum = ops.split_rhat(cm.mean, cm.m2, cm.n, mask, G.DIAG_RHAT_THRESHOLDS)
    poison((shape, torch.float32), (shape, torch.float32), ((5,), torch.float64))
    ess, mcse, esum = ops.split_ess(cm.mean, cm.m2, cm.vsum, cm.n, mask, G.DIAG_ESS_THRESHOLD)
    host = lambda t: t.cpu().numpy()
    return {'mean': host(cm.mean), 'm2': host(cm.m2), 'vsum': host(cm.vsum).astype(np.float64), 'ring': host(cm.ring), 'rhat': host(rhat),
            'rsum': rsum.tolist(), 'ess': host(ess), 'mcse': host(mcse), 'esum': esum.tolist()}


def check_variogram(t, x, shape, vsum, ring):
    from tests._split_ess import variogram_np
    with np.errstate(all='ignore'):
        ref = variogram_np(x, G.DIAG_LAG).reshape(vsum.shape)
    held(t, 'vsum', vsum, ref, 1e-5 * np.abs(ref))  # tests/test_gpu_ess.py:85-88
    N = x.shape[1]
    n = N // 2
    for k in range(max(1, n - G.DIAG_LAG + 1), n + 1):  # tests/test_gpu_ess.py:91-92: the ring holds the last samples, bit for bit
        assert np.array_equal(ring[(k - 1) % G.DIAG_LAG].reshape(x.shape[0], 3, -1).view(np.int32), x[:, N - n + k - 1].view(np.int32))


@functools.lru_cache(maxsize=None)
def small_chain_run(name):
    """the samples of a chain-update record that has a volume of its own, recorded -> (x, mean, m2, vsum, ring)"""
    rec = G.RECORD[name]
    x = G.diag_samples(rec.shape, 313, rec.chains, rec)[0]
    cm = record_chain(x, rec.shape)
    return x, cm.mean.cpu().numpy(), cm.m2.cpu().numpy(), cm.vsum.cpu().numpy().astype(np.float64), cm.ring.cpu().numpy()


def check_moments(t, x, mean, m2):
    """tests/test_gpu_chain_diagnostics.py:88-89: rtol 1e-5, atol 1e-5 (times n for M2), element by element; the one component with
    an infinite sample is non-finite on both sides"""
    mean_ref, m2_ref = moments_np(x)
    n = x.shape[1] // 2
    fin = np.isfinite(m2_ref)
    assert int((~fin).sum()) == 1
    got_mean, got_m2 = mean.reshape(mean_ref.shape), m2.reshape(m2_ref.shape)
    assert not np.isfinite(got_m2[~fin]).any()
    for half in (0, 1):
        held(t, f'mean, half {half}', got_mean[half][fin[half]], mean_ref[half][fin[half]], 1e-5 + 1e-5 * np.abs(mean_ref[half][fin[half]]))
        held(t, f'm2, half {half}', got_m2[half][fin[half]], m2_ref[half][fin[half]], 1e-5 * n + 1e-5 * np.abs(m2_ref[half][fin[half]]))


@pytest.mark.parametrize('name', G.records_of('diagnostics'))
def test_diagnostics(name):
    from tests._split_ess import ess_from_stats, var_plus_np
    rec, g = geometry_line(name)
    t = T(name)
    if 'chain_moments' in name:
        # <VEC>: two chains, both halves aligned.  <scalar>: C 3 V odd, so the state of half 1 (mean + C 3 V floats: api_ops.hip,
        # irs_chain_moments_update) is not 16-byte aligned and launch_chain_moments, which picks the form by alignment alone,
        # takes the scalar kernel for its four updates; half 0 takes the vector kernel and its scalar tail
        x, mean, m2, _, _ = small_chain_run(name)
        assert (x[0, 0].size * x.shape[0] * 4) % 16 == (0 if 'VEC' in name else 12)
        check_moments(t, x, mean, m2)
        return
    if 'scalar' in name:  # the scalar variogram: the samples and the run of the scalar moments record, E = 3 V odd
        x, _, _, vsum, ring = small_chain_run('diagnostics/chain_moments_kernel<scalar>')
        check_variogram(t, x, rec.shape, vsum, ring)
        return
    case, r = G.case('diagnostics/finalize'), diag_run()
    x, mask = case['x'], case['mask'].reshape(-1)
    Cn, V = x.shape[0], x.shape[-1]
    n = x.shape[1] // 2
    if 'variogram' in name:
        check_variogram(t, x, rec.shape, r['vsum'], r['ring'])
        check_moments(t + ' (moments of the same run: three trips)', x, r['mean'], r['m2'])
    elif 'rhat' in name:
        nbytes = C.c_size_t()  # the blocks the library itself counts (irs_split_rhat_workspace: 5 doubles per block)
        L.check(L.load().irs_split_rhat_workspace(Cn, *rec.shape, C.byref(nbytes)))
        assert nbytes.value == 5 * 8 * g.blocks
        got = r['rhat'].reshape(-1).astype(np.float64)
        held(t, 'rhat', got, case['rhat'], 2e-5 * np.abs(case['rhat']))  # tests/test_gpu_chain_diagnostics.py:52-58
        m = r['rhat'].reshape(-1)[mask]  # the summary: numpy on the returned map (tests/test_gpu_chain_diagnostics.py:61-65, 119-126)
        voxels, above0, above1, mx, total = r['rsum']
        same(t, 'voxels / above', [voxels, above0, above1], [m.size] + [int((m > np.float32(th)).sum()) for th in G.DIAG_RHAT_THRESHOLDS])
        held(t, 'max', mx, float(m.max()), 0)
        held(t, 'sum', total, float(m.astype(np.float64).sum()), 1e-12 * float(m.astype(np.float64).sum()))
        assert case['trip'][int(np.argmax(np.where(mask, got, -np.inf)))] == case['trip'].max()  # the largest R-hat sits in the last trip
    else:  # split ESS
        nbytes = C.c_size_t()
        L.check(L.load().irs_split_ess_workspace(Cn, *rec.shape, C.byref(nbytes)))
        assert nbytes.value == 5 * 8 * g.blocks
        with np.errstate(all='ignore'):  # tests/test_gpu_ess.py:53-57, 104-108: the restatement fed the device's own lag sums
            e4, s4, tr4, margin4 = ess_from_stats(var_plus_np(x), r['vsum'].reshape(G.DIAG_LAG, 3, V), 2 * x.shape[0], n, G.DIAG_LAG)
        e_ref, s_ref, tr_ref, margin = e4.min(axis=0), s4.max(axis=0), tr4.any(axis=0), margin4.min(axis=0)
        keep = margin >= 1e-6
        assert keep.mean() > 0.99
        held(t, 'ess', r['ess'].reshape(-1)[keep], e_ref[keep], 1e-5 * np.abs(e_ref[keep]))
        held(t, 'mcse', r['mcse'].reshape(-1)[keep], s_ref[keep], 1e-5 * np.abs(s_ref[keep]))
        e = r['ess'].reshape(-1)[mask]  # the summary: numpy on the returned maps (tests/test_gpu_ess.py:149-159)
        voxels, below, truncated, mn, total = r['esum']
        same(t, 'voxels / below', [voxels, below], [e.size, int((e < np.float32(G.DIAG_ESS_THRESHOLD)).sum())])
        assert 0 < below < voxels
        assert keep[mask].all()  # no truncation decision under the mask is on a knife edge (tests/_grid_caps.py leaves those out)
        same(t, 'truncated', truncated, int(tr_ref[mask].sum()))  # tests/test_gpu_ess.py:152-156
        held(t, 'min', mn, float(e.min()), 0)
        held(t, 'sum', total, float(e.astype(np.float64).sum()), 1e-12 * float(e.astype(np.float64).sum()))


# ---------------------------------------------------------------- inverse consistency
def residual_bound(t_a, d_a, d_b):
    """tests/test_gpu_inverse_consistency.py:100-110, the per-element bound derived there"""
    from tests import _inverse_consistency as R
    Cn, _, D, H, W = d_b.shape
    b = d_b.double()
    slope = [(b[..., :, :, 1:] - b[..., :, :, :-1]).abs().amax(dim=(2, 3, 4)), (b[..., :, 1:, :] - b[..., :, :-1, :]).abs().amax(dim=(2, 3, 4)),
             (b[..., 1:, :, :] - b[..., :-1, :, :]).abs().amax(dim=(2, 3, 4))]
    position = sum(3 * U * (n - 1) * s for n, s in zip((W, H, D), slope)).view(Cn, 3, 1, 1, 1)
    S = R.tap_weight_sum(t_a, d_b)
    return position + 11 * U * S + U * (d_a.double().abs() + S)


def stream_records(rec, seed, lo=0.0):
    """two recorded steps of per-voxel maps (2, C, 1, *shape) float32 for a per-voxel update kernel: the later trips on another
    level and spread; in the last trip a voxel that is NaN in some records and one that is NaN in all of them"""
    trip, block, g = G.trips_of(rec)
    rng = np.random.default_rng(seed)
    maps = ((rng.random((2, rec.chains, g.elements)) * (2.0 - lo) + lo) * (1 + trip) * 0.25 + 0.125 * trip).astype(np.float32)
    some, never = G._last(trip, 3), G._last(trip, 4)
    maps[0, 0, some] = maps[1, -1, some] = np.nan
    maps[:, :, never] = np.nan
    return maps.reshape(2, rec.chains, 1, *rec.shape), some, never


@pytest.mark.parametrize('name', G.records_of('inverse_consistency'))
def test_inverse_consistency(name):
    from tests import _inverse_consistency as R
    rec, g = geometry_line(name)
    t = T(name)
    Cn, shape = rec.chains, rec.shape
    if name.endswith('inverse_consistency_kernel'):
        case = G.case('inverse_consistency/main')
        poison(((Cn, 1, *shape), torch.float32), ((Cn, 3, *shape), torch.float32), ((Cn, 2), torch.int64), ((Cn, 3), torch.float64))
        norm, res, isum, fsum = ops.inverse_consistency(dev(case['t_a']), dev(case['d_a']), dev(case['d_b']), mask=dev(case['mask']),
                                                        want_residual=True)
        bound = residual_bound(case['t_a'], case['d_a'], case['d_b'])  # tests/test_gpu_inverse_consistency.py:134-139
        r64, n64 = case['r64'], case['n64']
        bound = torch.nan_to_num(bound, nan=0.0, posinf=0.0)  # (where an input is not finite neither is the reference: not compared)
        held(t, 'residual', res.cpu().numpy(), r64.numpy(), bound.numpy())
        nbound = torch.sqrt((bound * bound).sum(dim=1, keepdim=True)) + 4 * U * torch.nan_to_num(n64, nan=0.0, posinf=0.0)
        held(t, 'norm', norm.cpu().numpy(), n64.numpy(), nbound.numpy())
        isum, fsum, norm = isum.cpu(), fsum.cpu(), norm.cpu()
        for c in range(Cn):  # the summary of the stored map (tests/test_gpu_inverse_consistency.py:74-81)
            ints, floats = R.chain_summary(norm[c, 0], case['mask'][c, 0])
            same(t, f'chain {c} counts', isum[c].tolist(), ints)
            n = max(ints[0], 1)
            held(t, f'chain {c} sum', float(fsum[c, 0]), floats[0], n * 2.0 ** -53 * floats[0])
            held(t, f'chain {c} sum of squares', float(fsum[c, 1]), floats[1], n * 2.0 ** -53 * floats[1])
            held(t, f'chain {c} max', float(fsum[c, 2]), floats[2], 0)
        assert isum[:, 1].tolist() == [0, 2]
    elif 'update' in name:
        recs, some, never = stream_records(rec, 21)
        mean, peak = torch.full(shape, float('nan'), device=DEV), torch.full(shape, float('nan'), device=DEV)
        state = None
        for i in range(2):  # records_before = 0, then > 0
            ops.inverse_consistency_update(dev(recs[i]), mean, peak, i * Cn)
            state = R.update(state, torch.from_numpy(recs[i]), i * Cn, torch.float64)
        m64, p64 = state
        assert int(torch.isnan(m64).sum()) == 2 and int(torch.isnan(p64).sum()) == 1
        top = float(np.nanmax(recs))
        held(t, 'mean', mean.cpu().numpy(), m64.numpy(), 6 * 2 * Cn * U * top)  # tests/test_gpu_inverse_consistency.py:169-171, 194
        held(t, 'peak', peak.cpu().numpy(), p64.numpy(), 0)
    elif 'negate' in name:
        trip, _, _ = G.trips_of(rec)
        v = dev(R.smooth_field(Cn, shape, 4.0, 5) * torch.from_numpy((1.0 + trip).reshape(Cn, 3, *shape)).float())
        t_inv, d_inv = ops.svf_exp_inverse(v, 2)      # tests/test_gpu_inverse_consistency.py:39-44
        t_ref, d_ref, _ = ops.svf_exp_fwd(-v, 2)
        held(t, 'inverse transformation', t_inv.cpu().numpy(), t_ref.cpu().numpy(), 0)
        held(t, 'inverse displacement', d_inv.cpu().numpy(), d_ref.cpu().numpy(), 0)
        assert float(d_inv.abs().max()) > 0
    else:
        case = G.case('inverse_consistency/finalize')
        poison(((3,), torch.int64), ((3,), torch.float64))
        isum, fsum = ops.inverse_consistency_finalize(dev(case['mean']), dev(case['peak']), G.ICE_THRESHOLD, dev(case['mask']))
        ints, floats = R.map_summary(torch.from_numpy(case['mean']), torch.from_numpy(case['peak']), G.ICE_THRESHOLD,
                                     torch.from_numpy(case['mask']))
        same(t, 'counts', isum.tolist(), ints)  # tests/test_gpu_inverse_consistency.py:197-200
        held(t, 'sum of the mean', float(fsum[0]), floats[0], ints[0] * 2.0 ** -53 * floats[0])
        held(t, 'maxima', fsum[1:].tolist(), floats[1:], 0)
        assert ints[1] == 2 and 0 < ints[2] < ints[0]


# ---------------------------------------------------------------- local similarity
@pytest.mark.parametrize('name', G.records_of('local_similarity'))
def test_local_similarity(name):
    from tests import _local_similarity as S
    rec, g = geometry_line(name)
    t = T(name)
    Cn, shape = rec.chains, rec.shape
    if '<1>' in name:
        case = G.case('local_similarity/main')
        poison(((Cn, 1, *shape), torch.float32), ((Cn, 1, *shape), torch.float32), ((Cn, L.IRS_LOCAL_STATS), torch.float64))
        out = ops.local_similarity(dev(case['fixed']), dev(case['moving']), dev(case['mask'])[None, None], 1, S.UNIT, S.UNIT)
        got = {k: v.cpu().numpy() for k, v in out.items()}
        for c, ref in enumerate(case['maps']):  # tests/test_gpu_local_similarity.py:64-80
            for key_, bound in (('lncc', S.lncc_bound(ref)), ('ssim', S.ssim_bound(ref))):
                with np.errstate(invalid='ignore'):
                    held(t, f'{key_} chain {c}', got[key_][c, 0], ref[key_], np.nan_to_num(bound, nan=0.0, posinf=0.0))
        want = np.array([[S.reference_stats(ref, case['mask'])[k] for k in S.COLUMNS] for ref in case['maps']], dtype=np.float64)
        same(t, 'counts', got['stats'][:, :3], want[:, :3])  # tests/test_gpu_local_similarity.py:83-93
        for j, k in enumerate(S.COLUMNS[3:], 3):
            held(t, k, got['stats'][:, j], want[:, j], 1e-9)
        assert want[1, 2] > 0 and (want[:, 4] < -0.99).all()
    elif 'update' in name:
        recs, some, never = stream_records(rec, 31, lo=-2.0)
        recs = np.clip(recs / np.nanmax(np.abs(recs)), -1.0, 1.0).astype(np.float32)  # LNCC-like: |x| <= 1
        mean, low = torch.full(shape, float('nan'), device=DEV), torch.full(shape, float('nan'), device=DEV)
        count = torch.full(shape, -7, device=DEV, dtype=torch.int32)
        for i in range(2):
            ops.local_similarity_update(dev(recs[i]), mean, low, count, i * Cn)
        K = 2 * Cn
        flat = recs.reshape((K,) + shape).astype(np.float64)  # tests/test_gpu_local_similarity.py:242-262: a two-pass reference
        n_ref = (~np.isnan(flat)).sum(0)
        with np.errstate(invalid='ignore', divide='ignore'):
            mean_ref = np.where(n_ref > 0, np.nansum(flat, 0) / n_ref, np.nan)
        low_ref = np.where(n_ref > 0, np.min(np.where(np.isnan(flat), np.inf, flat), 0), np.nan)
        same(t, 'count', count.cpu().numpy(), n_ref)
        some_ = n_ref > 0
        assert int((~some_).sum()) == 1 and int((n_ref == K - 2).sum()) == 1
        held(t, 'mean', mean.cpu().numpy()[some_], mean_ref[some_], 5 * K * U)
        held(t, 'low', low.cpu().numpy()[some_], low_ref[some_], 0)
    else:
        case = G.case('local_similarity/finalize')
        poison(((2,), torch.int64), ((3,), torch.float64))
        isum, fsum = ops.local_similarity_finalize(dev(case['mean']), dev(case['low']), dev(case['count']), dev(case['mask']))
        want = case['reference'](np.ones(case['trip'].size, np.int64))  # sums over the stored maps (tests/test_gpu_local_similarity.py:265-270)
        same(t, 'counts', isum.tolist(), [want['voxels'], want['empty']])
        held(t, 'sum of the mean', float(fsum[0]), want['sum_mean'], case['tol']['sum_mean'])
        held(t, 'minima', fsum[1:].tolist(), [want['min_mean'], want['min_low']], 0)
        assert want['empty'] == 3


# ---------------------------------------------------------------- residual check
def compare_residual(t, got, want, zs, m):
    """tests/test_gpu_residual_check.py:55-70: integers and the maximum equal; the sums to 4 n 2^-53 of their sums of magnitudes"""
    (hist, counts, sums), (rh, rc, rs) = got, want
    same(t, 'hist', hist, rh)
    same(t, 'counts', counts, rc)
    held(t, 'max |z|', sums[:, 3], rs[:, 3], 0)
    for c in range(hist.shape[0]):
        d = np.concatenate([z[c][m & np.isfinite(z[c])] for z in zs]).astype(np.float64)
        rel = G.RES_MARGIN * max(d.size, 1) * 2.0 ** -53
        for j, mag in enumerate((math.fsum(np.abs(d)), math.fsum(d * d), math.fsum((d * d) ** 2))):
            held(t, f'chain {c} sum {j}', sums[c, j], rs[c, j], rel * mag)


@pytest.mark.parametrize('name', G.records_of('residual_check'))
def test_residual_check(name):
    from tests import _residual_check as S
    rec, g = geometry_line(name)
    t = T(name)
    Cn, shape = rec.chains, rec.shape
    if 'histogram' in name:
        case = G.case('residual_check/histogram ' + ('vector' if 'VEC' in name else 'scalar'))
        zs, m = case['steps'], case['mask']
        five = lambda a: a.reshape(a.shape[0], 1, *shape)
        refs = [S.reference_histogram(five(z), m.reshape(1, 1, *shape), G.RES_HALF, G.RES_BINS) for z in zs]
        want = S.accumulate(refs[0], refs[1])
        assert (want[1][:, 1] > 0).all() and (want[1][:, 2] > 0).all()
        md = dev(m.reshape(1, 1, *shape))
        try:
            for aggregate in (1, 0):
                L.option_set('similarity_aggregate', aggregate)
                poison(((Cn, G.RES_BINS), torch.int64), ((Cn, 3), torch.int64), ((Cn, 4), torch.float64))
                state = RC.residual_histogram(dev(five(zs[0])), md, G.RES_HALF, G.RES_BINS)  # records_before = 0, then > 0
                state = RC.residual_histogram(dev(five(zs[1])), md, G.RES_HALF, G.RES_BINS, **state, records_before=Cn)
                compare_residual(f'{t} aggregate {aggregate}', tuple(state[k].cpu().numpy() for k in ('hist', 'counts', 'sums')), want, zs, m)
        finally:
            L.option_set('similarity_aggregate', 1)
    elif 'update' in name:
        trip, _, _ = G.trips_of(rec)
        records, models = [], []
        rng = np.random.default_rng(4)
        for r in range(2):  # tests/test_gpu_residual_check.py:163-189
            std = np.exp(np.linspace(math.log(0.01), math.log(1.0), 4)) * (1.0 + 0.1 * r)
            pi = rng.dirichlet(np.ones(4))
            z = (S.draw_mixture((g.elements,), Cn, std, pi, seed=40 + r).reshape(Cn, -1) * (1 + 2 * trip) + 0.1 * trip).astype(np.float32)
            z[0, G._last(trip, 3 + r)] = np.nan
            z[1, G._last(trip, 5)] = (np.inf, -np.inf)[r]
            z[1, G._last(trip, 6)] = 60.0
            z[:, G._last(trip, 7)] = np.nan
            records.append(z.reshape(Cn, 1, *shape))
            models.append(S.mixture_terms(std, pi))
        mean, count = torch.full(shape, float('nan'), device=DEV), torch.full(shape, -7, device=DEV, dtype=torch.int32)
        for r, (z, (lw, inv)) in enumerate(zip(records, models)):
            RC.residual_nll_update(dev(z), lw, inv, mean, count, Cn * r)
        want_mean, want_count, biggest = S.reference_nll_map(records, models)
        same(t, 'count', count.cpu().numpy(), want_count)
        assert want_count.min() == 0 and want_count.max() == 2 * Cn
        some = want_count > 0
        harmonic = sum(1.0 / k for k in range(1, 2 * Cn + 1))  # nll_bound of tests/test_gpu_residual_check.py:153-160
        held(t, 'mean NLL', mean.cpu().numpy()[some], want_mean[some], U * biggest * (2 * Cn + 4.0 * harmonic + 1.0))
        assert float(mean.cpu().numpy()[~some].max()) == 0.0
    else:
        case = G.case('residual_check/finalize')
        poison(((2,), torch.int64), ((2,), torch.float64))
        isum, fsum = RC.residual_nll_finalize(dev(case['mean']), dev(case['count']), dev(case['mask']))
        wi, wf = S.reference_nll_summary(case['mean'], case['count'], case['mask'])  # tests/test_gpu_residual_check.py:191-194
        same(t, 'counts', isum.tolist(), wi)
        held(t, 'max of the mean', fsum[1].item(), wf[1], 0)
        held(t, 'sum of the mean', fsum[0].item(), wf[0], case['tol']['sum_mean'])
        assert wi[1] == 3


# ---------------------------------------------------------------- image similarity
@pytest.mark.parametrize('name', G.records_of('image_similarity'))
def test_image_similarity(name):
    from tests import _image_similarity as S
    rec, g = geometry_line(name)
    case = G.case('image_similarity/' + name.split('<')[1])
    Cn, shape = rec.chains, rec.shape
    five = lambda a: a.reshape(-1, 1, *shape)
    fixed, moving, mask = five(case['fixed']), five(case['moving']), case['mask'].reshape(1, 1, *shape)
    hist, stats = S.reference(fixed, moving, mask, G.SIM_BINS, G.SIM_UNIT, G.SIM_UNIT)
    COL = {k: j for j, k in enumerate(S.COLUMNS)}
    assert (stats[:, COL['n_nonfinite']] > 0).all() and (stats[:, COL['n_clipped']] > 0).all()
    fd, md, kd = dev(fixed), dev(moving), dev(mask)
    try:
        for aggregate in (1, 0):
            L.option_set('similarity_aggregate', aggregate)
            t = T(f'{name} aggregate {aggregate}')
            poison(((Cn, L.IRS_SIMILARITY_STATS), torch.float64), ((Cn, G.SIM_BINS, G.SIM_BINS), torch.int32))
            out = ops.image_similarity(fd, md, kd, G.SIM_BINS, G.SIM_UNIT, G.SIM_UNIT, want_hist=True)
            got = {k: v.cpu().numpy() for k, v in out.items()}
            same(t, 'hist', got['hist'], hist)  # tests/test_gpu_image_similarity.py:59-69
            same(t, 'counts', got['stats'][:, :3], stats[:, :3])
            held(t, 'mse', got['stats'][:, COL['mse']], stats[:, COL['mse']], 1e-9 * stats[:, COL['mse']])
            for k in S.COLUMNS[4:]:
                held(t, k, got['stats'][:, COL[k]], stats[:, COL[k]], 1e-9)
    finally:
        L.option_set('similarity_aggregate', 1)


# ---------------------------------------------------------------- label posterior
@functools.lru_cache(maxsize=None)
def label_reference():
    from tests._label_posterior import label_posterior_np
    case = G.case('label_posterior/scalar')
    shape = case['record'].shape
    n = case['records'].shape[0]
    return label_posterior_np(case['records'].reshape(n, *shape), case['fixed'].reshape(shape), list(case['labels']), case['mask'].reshape(shape))


def label_updates(case, rec, labels):
    """the recorded steps through ops.label_posterior_update: records_before = 0, then > 0 -> (counts, volume)"""
    n, K = case['records'].shape[0], len(labels)
    counts = torch.zeros((K, *rec.shape), device=DEV, dtype=torch.int32)             # an accumulator: it has to start at zero
    volume = torch.full((K, 2), float('nan'), device=DEV, dtype=torch.float64)       # the first record overwrites it
    seg = dev(case['records'].reshape(n // rec.chains, rec.chains, 1, *rec.shape))
    for s in range(n // rec.chains):
        ops.label_posterior_update(seg[s], list(labels), counts, volume, s * rec.chains)
    return counts.cpu().numpy(), volume.cpu().numpy()


@pytest.mark.parametrize('name', G.records_of('label_posterior'))
def test_label_posterior(name):
    rec, g = geometry_line(name)
    t = T(name)
    if 'VEC' in name:
        case = G.case('label_posterior/vector')
        assert g.elements % 8 == 0
        counts, volume = label_updates(case, rec, case['labels'])
        want = case['reference'](np.ones(g.elements, np.int64))
        for j, lab in enumerate(case['labels']):
            same(t, f'counts of label {lab}', counts[j].reshape(-1), (case['records'] == lab).sum(axis=0))
            for col, k in enumerate(('vol_mean', 'vol_m2')):  # tests/test_gpu_label_posterior.py:46-48
                held(t, f'{k} of label {lab}', volume[j, col], want[f'{j}/{k}'], 1e-12 * max(abs(want[f'{j}/{k}']), 1e-300))
        return
    case, ref = G.case('label_posterior/scalar'), label_reference()
    labels = list(case['labels'])
    if 'update' in name:
        counts, volume = label_updates(case, rec, labels)
        same(t, 'counts', counts, ref['counts'])  # tests/test_gpu_label_posterior.py:41-48
        for col, k in enumerate(('vol_mean', 'vol_m2')):
            held(t, k, volume[:, col], ref[k], 1e-12 * np.maximum(np.abs(ref[k]), 1e-300))
    else:
        K = len(labels)
        poison((rec.shape, torch.float32), (rec.shape, torch.int16), ((K, 6 + 3 * L.IRS_LABEL_BINS), torch.int64), ((4,), torch.float64))
        entropy, map_label, summary, mask_summary = ops.label_posterior_finalize(dev(ref['counts'].astype(np.int32)), ref['n'], labels,
                                                                                 dev(case['fixed'].reshape(rec.shape)),
                                                                                 dev(case['mask'].reshape(rec.shape)))
        same(t, 'MAP label', map_label.cpu().numpy(), ref['map'])  # tests/test_gpu_label_posterior.py:41-58
        held(t, 'entropy', entropy.cpu().numpy(), ref['entropy'], 1e-6)
        same(t, 'summary', summary.cpu().numpy(), ref['summary'])
        voxels, esum, emax, bad = mask_summary.tolist()
        same(t, 'voxels / inconsistent', [voxels, bad], [ref['entropy_voxels'], 0])
        held(t, 'entropy sum', esum, ref['entropy_sum'], 1e-6 * ref['entropy_voxels'])
        held(t, 'entropy max', emax, ref['entropy_max'], 1e-6)
        assert abs(ref['entropy_max'] - math.log(4.0)) < 1e-6


# ---------------------------------------------------------------- surface posterior
@pytest.mark.parametrize('name', G.records_of('surface_posterior'))
def test_surface_posterior(name):
    from tests import _surface_posterior as S
    rec, g = geometry_line(name)
    t = T(name)
    case = G.case('surface_posterior/finalize')
    labels = list(S.LABELS3)
    poison((rec.shape, torch.float32), (rec.shape, torch.float32), ((3, L.IRS_SURFACE_SUMMARY_INTS), torch.int64),
           ((3, L.IRS_SURFACE_SUMMARY_FLOATS), torch.float64))
    bias, std, isum, fsum = ops.surface_posterior_finalize(dev(case['seg'])[None, None], labels, dev(case['mean']), dev(case['m2']),
                                                           dev(case['count']), G.SURF_LEVELS, dev(case['mask']))
    bias, std, isum, fsum = bias.cpu().numpy(), std.cpu().numpy(), isum.cpu().numpy(), fsum.cpu().numpy()
    held(t, 'bias', bias, case['bias'], 0)                                                     # the stored mean itself
    # tests/_surface_posterior.py:21-23: the division and the root round by at most 2 u std together, held to 4 u std
    held(t, 'std', std, case['std'], 4 * U * np.nan_to_num(case['std'].astype(np.float64)))
    # the summary of the maps the device stored (tests/_surface_posterior.py:262-268: integers equal, the coverage columns from the call's own maps)
    want_i, want_f = S.summary(bias, std, case['count'], case['seg'], labels, G.SURF_LEVELS, case['mask'])
    nl = len(G.SURF_LEVELS)
    same(t, 'integer columns', isum[:, :3 + nl], want_i)
    assert not isum[:, 3 + nl:].any() and (want_i[:, :3] > 0).all()
    for j in range(3):
        for k in range(6):
            held(t, f'label {j} float column {k}', fsum[j, k], want_f[j, k], case['tol'][f'{j}/f{k}'])


# ---------------------------------------------------------------- masks
@pytest.mark.parametrize('name', G.records_of('masks'))
def test_masks(name):
    from tests import _masks as S
    rec = G.RECORD[name]
    t = T(name)
    shape = rec.shape
    if 'histogram' in name:
        geometry_line(name)
        case = G.case('masks/histogram')
        five = lambda a: a.reshape(rec.chains, 1, *shape)
        poison(((rec.chains, G.MASK_BINS), torch.int64))
        h = M.intensity_histogram(dev(five(case['im'])), G.MASK_BINS, G.MASK_RANGE, dev(five(case['mask']))).cpu().numpy()
        for c in range(rec.chains):  # tests/test_gpu_masks.py:283-287
            same(t, f'histogram of volume {c}', h[c], S.intensity_histogram(case['im'][c], G.MASK_BINS, G.MASK_RANGE, case['mask'][c]))
        return
    comp = G.case('masks/components')
    volumes = dev(comp['volumes'])[:, None]
    if 'scan' in name:
        g = G.geometry(rec)
        print(f'{name}: shape {shape}: {g.units} chunks, {g.trips} per thread')
        assert g.trips == 2
        poison(((rec.chains, 1, *shape), torch.int32), ((rec.chains,), torch.int32))
        labels, counts = M.connected_components(volumes, 26)
        labels, counts = labels[:, 0].cpu().numpy(), counts.cpu().numpy()
        for c in range(rec.chains):  # tests/test_gpu_masks.py:48-56, the labels compared canonically
            same(t, f'components of volume {c}', counts[c], comp['sizes'][c].size)
            same(t, f'labels of volume {c}', S.canonical_labels(labels[c]), comp['labels'][c])
    else:
        n = comp['sizes'][0].size
        print(f'{name}: shape {shape}: {n} components, {-(-n // 1024)} sweep trips')
        assert n > 1024
        for keep in (1, 3):  # tests/test_gpu_masks.py:146-152
            poison(((rec.chains, 1, *shape), torch.uint8))
            out = M.keep_largest(volumes, 26, keep)[:, 0].cpu().numpy()
            for c in range(rec.chains):
                want = np.isin(comp['labels'][c], G.kept_components(comp['sizes'][c], keep))
                same(t, f'keep {keep} of volume {c}', out[c], want)
                assert int(want.sum()) == (60, 60 + 59 + 58)[keep == 3]


def test_every_record_is_in_a_parametrisation():
    names = []
    for family in G.FAMILIES:
        names += G.records_of(family)
    assert sorted(names) == sorted(G.RECORD) and len(names) == len(G.RECORDS)
