"""The residual model check on the GPU (residual_check.residual_histogram / residual_nll_update / residual_nll_finalize,
utils.calc_residual_check, the trainer's `residual_check` option) against the numpy restatement of tests/_residual_check.py,
which shares no code with the HIP path.

The histogram and the three counts are integers and must be EQUAL: the binning is stated in float32 operations that numpy
repeats bit for bit.  max |z| is a maximum of exact conversions: equal.  The three sums are double sums of n terms: summing n
terms in any order moves the result by at most (n - 1) 2^-53 sum |x| (Higham, Accuracy and Stability, eq. 4.4), z^2 is exact in
double and z^4 carries one more rounding per term; the restatement sums exactly (math.fsum).  The bound used is SUM_MARGIN n
2^-53 sum |x| with SUM_MARGIN = 4 for that extra rounding, FMA contraction and the merge of two calls."""
import copy
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

from ir_sgmcmc_amd import _lib as L
from ir_sgmcmc_amd import residual_check as R
from ir_sgmcmc_amd.utils import calc_residual_check
from tests import _residual_check as S

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUM_MARGIN = 4.0
STD, PI, HALF = (0.05, 0.2), (0.7, 0.3), 0.5

ODD, VEC, BIG = (5, 7, 9), (4, 8, 16), (17, 16, 65)  # 315 voxels (scalar path); the 16-byte path; 17 680: several blocks per chain
# (shape, C, mask, bins, kind): every value of every axis appears
SWEEP = [(ODD, 1, None, 2, 'mix'), (ODD, 2, 'bool', 37, 'mix'), (ODD, 2, 'uint8', 128, 'spoiled'), (ODD, 1, 'bool', 512, 'flat'),
         (VEC, 1, 'bool', 128, 'mix'), (VEC, 2, None, 37, 'spoiled'), (VEC, 2, 'uint8', 2, 'flat'), (VEC, 2, 'bool', 512, 'mix'),
         (BIG, 2, 'bool', 128, 'mix'), (BIG, 1, 'uint8', 37, 'spoiled'), (BIG, 2, None, 512, 'flat'), (BIG, 2, 'bool', 2, 'spoiled'),
         (BIG, 1, None, 128, 'flat')]


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(out):
    return tuple(out[k].cpu().numpy() for k in ('hist', 'counts', 'sums'))


def build(shape, C, mask, kind, seed):
    m = None if mask is None else S.random_mask(shape, seed + 2, bool if mask == 'bool' else np.uint8)
    z = (S.flat_background if kind == 'flat' else S.draw_mixture)(shape, C, STD, PI, seed)
    if kind == 'spoiled':
        z = S.spoil(z, m, HALF, seed + 1)
    return z, m


def compare(name, got, want, z, m):
    """integers and the maximum equal; the sums to SUM_MARGIN n 2^-53 of their sums of magnitudes"""
    (hist, counts, sums), (rh, rc, rs) = got, want
    assert hist.dtype == np.int64 and counts.dtype == np.int64 and sums.dtype == np.float64
    assert (hist == rh).all(), name
    assert (counts == rc).all(), (name, counts, rc)
    assert (sums[:, 3] == rs[:, 3]).all(), (name, sums[:, 3], rs[:, 3])
    mm = np.ones(z[0].size, bool) if m is None else m.reshape(-1) != 0
    for c in range(z.shape[0]):
        zc = z[c].reshape(-1)
        d = zc[mm & np.isfinite(zc)].astype(np.float64)
        rel = SUM_MARGIN * max(len(d), 1) * 2.0 ** -53
        for j, mag in enumerate((math.fsum(np.abs(d)), math.fsum(d * d), math.fsum((d * d) ** 2))):
            dev_ = abs(sums[c, j] - rs[c, j])
            print(f'{name} chain {c} sum {j}: deviation {dev_:.3e}, bound {rel * mag:.3e}')
            assert dev_ <= rel * mag, (name, c, j, sums[c, j], rs[c, j])


@pytest.mark.parametrize('shape,C,mask,bins,kind', SWEEP)
def test_histogram_against_the_restatement(shape, C, mask, bins, kind):
    z, m = build(shape, C, mask, kind, seed=sum(shape) + C + bins)
    want = S.reference_histogram(z, m, HALF, bins)
    got = host(R.residual_histogram(dev(z), dev(m), HALF, bins))
    assert got[0].shape == (C, bins) and got[1].shape == (C, 3) and got[2].shape == (C, 4)
    if kind == 'spoiled':
        assert (want[1][:, 1] > 0).all() and (want[1][:, 2] > 0).all()
    if kind == 'flat':  # at least half of the voxels taking part in ONE bin: whole wavefronts add their number with one lane
        assert (2 * want[0].max(axis=1) >= want[1][:, 0]).all() and want[1][0, 0] > 100
    compare(f'{shape} C={C} {mask} bins={bins} {kind}', got, want, z, m)


def test_plain_atomics_count_the_same():
    z, m = build(BIG, 2, 'bool', 'flat', seed=3)
    zd, md = dev(z), dev(m)
    a = R.residual_histogram(zd, md, HALF, 64)
    L.option_set('similarity_aggregate', 0)
    try:
        b = R.residual_histogram(zd, md, HALF, 64)
    finally:
        L.option_set('similarity_aggregate', 1)
    assert all(torch.equal(a[k].view(torch.int64), b[k].view(torch.int64)) for k in a)
    empty = host(R.residual_histogram(zd, dev(np.zeros((1, 1, *BIG), bool)), HALF, 64))
    assert not empty[0].any() and not empty[1].any() and (empty[2][:, :3] == 0).all() and (empty[2][:, 3] == -np.inf).all()


def test_bin_edges():
    """z == half_range is in the last bin and not clipped; the next float is clipped; -half_range opens bin 0"""
    h = np.float32(HALF)
    vals = np.array([-h, np.nextafter(-h, np.float32(-1)), 0.0, np.nextafter(np.float32(0), np.float32(-1)), h,
                     np.nextafter(h, np.float32(1)), 0.25, -0.25], np.float32)
    z = vals.reshape(1, 1, 2, 2, 2)
    hist, counts, sums = host(R.residual_histogram(dev(z), None, HALF, 8))
    # (the float below 0 rounds to h when h is added: bin 4 with 0 itself)
    assert hist[0].tolist() == [2, 0, 1, 0, 2, 0, 1, 2] and counts[0].tolist() == [8, 0, 2]
    want = S.reference_histogram(z, None, HALF, 8)
    assert (hist == want[0]).all() and (counts == want[1]).all() and sums[0, 3] == float(np.nextafter(h, np.float32(1)))


# ---------------------------------------------------------------- accumulation, determinism
def test_accumulation_over_calls():
    z1, m = build(BIG, 2, 'bool', 'mix', seed=11)
    z2 = S.spoil(S.draw_mixture(BIG, 2, STD, PI, seed=12), m, HALF, seed=13)
    md = dev(m)
    state = R.residual_histogram(dev(z1), md, HALF, 37)
    state = R.residual_histogram(dev(z2), md, HALF, 37, **state, records_before=2)
    want = S.accumulate(S.reference_histogram(z1, m, HALF, 37), S.reference_histogram(z2, m, HALF, 37))
    z12 = np.concatenate([z1, z2], axis=2)  # the magnitudes of both calls bound the merged sums
    m12 = np.concatenate([m, m], axis=2)
    compare('two calls', host(state), want, z12, m12)
    # records_before = 0 over a dirty state is a call over a fresh one
    dirty = {'hist': torch.full((2, 37), 7, device=DEV, dtype=torch.int64), 'counts': torch.full((2, 3), -3, device=DEV, dtype=torch.int64),
             'sums': torch.full((2, 4), math.nan, device=DEV, dtype=torch.float64)}
    over, fresh = R.residual_histogram(dev(z1), md, HALF, 37, **dirty), R.residual_histogram(dev(z1), md, HALF, 37)
    assert all(torch.equal(over[k].view(torch.int64), fresh[k].view(torch.int64)) for k in fresh)


def test_determinism_chains_and_unaligned_bases():
    z, m = build(BIG, 2, 'uint8', 'mix', seed=21)
    zd, md = dev(z), dev(m)
    bits = lambda t: t.view(torch.int64)
    a, b = R.residual_histogram(zd, md, HALF, 128), R.residual_histogram(zd, md, HALF, 128)
    assert all(torch.equal(bits(a[k]), bits(b[k])) for k in a)
    for c in range(2):  # chain c of the two-chain call is the one-chain call on that chain, bit for bit
        one = R.residual_histogram(zd[c:c + 1].contiguous(), md, HALF, 128)
        assert all(torch.equal(bits(a[k][c:c + 1]), bits(one[k])) for k in a), c
    # V % 4 == 0 but the base 4 bytes off a 16-byte boundary: the scalar path counts the same voxels
    z, m = build(VEC, 2, 'bool', 'mix', seed=22)
    V = int(np.prod(VEC))
    buf = torch.zeros(2 * V + 1, device=DEV)
    buf[1:] = dev(z).reshape(-1)
    view = buf[1:].view(2, 1, *VEC)
    assert view.data_ptr() % 16 == 4
    al, off = R.residual_histogram(dev(z), dev(m), HALF, 37), R.residual_histogram(view, dev(m), HALF, 37)
    assert torch.equal(al['hist'], off['hist']) and torch.equal(al['counts'], off['counts']) and torch.equal(al['sums'][:, 3], off['sums'][:, 3])
    compare('unaligned base', host(off), S.reference_histogram(z, m, HALF, 37), z, m)


# ---------------------------------------------------------------- the NLL map
def nll_bound(n_max, biggest):
    """|float32 recursion - float64 running mean| per voxel.  The input: nll rounded once to float32, u = 2^-24 relative, and a
    mean of values each off by at most u M is off by at most u M (M = max |nll|).  Update k makes three roundings: d = nll -
    mean (|d| <= 2 M, its error divided by k), q = d / k (|q| <= 2 M / k) and the sum (|mean| <= M): at most u M (4 / k + 1); an
    earlier error is carried on with the factor 1 - 1/k <= 1.  Summed over k = 1 .. N: u M (N + 4 H_N), H_N the harmonic number.
    Together u M (N + 4 H_N + 1); the float64 exp / log of the device against numpy's is eight orders below."""
    harmonic = sum(1.0 / k for k in range(1, n_max + 1))
    return 2.0 ** -24 * biggest * (n_max + 4.0 * harmonic + 1.0)


@pytest.mark.parametrize('shape,K,mask', [(ODD, 1, None), (VEC, 4, 'bool'), (BIG, 8, 'uint8')])
def test_nll_map_against_the_restatement(shape, K, mask):
    rng = np.random.default_rng(K)
    records, models = [], []
    for r in range(3):
        std = np.exp(np.linspace(math.log(0.01), math.log(1.0), K)) * (1.0 + 0.1 * r)
        pi = rng.dirichlet(np.ones(K))
        z = S.draw_mixture(shape, 2, std, pi, seed=10 * K + r)
        flat = z.reshape(2, -1)
        flat[0, r::5] = np.nan  # skipped, and counted per voxel
        flat[1, 3::7] = (np.inf, -np.inf)[r % 2]
        flat[1, 1] = 60.0  # |z| / sigma_min = 6000: exp(-1.8e7) underflows, the sum must not
        flat[:, 2] = np.nan  # never finite at this voxel
        records.append(z)
        models.append(S.mixture_terms(std, pi))
    assert np.exp(models[0][0][0] - 0.5 * (60.0 * models[0][1][0]) ** 2) == 0.0
    mean, count = torch.full(shape, 9.0, device=DEV), torch.full(shape, 5, device=DEV, dtype=torch.int32)  # dirty: 0 overwrites
    for r, (z, (lw, inv)) in enumerate(zip(records, models)):
        R.residual_nll_update(dev(z), lw, inv, mean, count, 2 * r)
    want_mean, want_count, biggest = S.reference_nll_map(records, models)
    got_mean, got_count = mean.cpu().numpy(), count.cpu().numpy()
    assert (got_count == want_count).all() and want_count.reshape(-1)[2] == 0 and want_count.max() == 6 and want_count.min() == 0
    assert got_mean.reshape(-1)[2] == 0.0 and np.isfinite(got_mean).all()
    some = want_count > 0
    dev_, bound = float(np.abs(got_mean[some] - want_mean[some]).max()), nll_bound(6, biggest)
    print(f'{shape} K={K}: max |nll| {biggest:.4g}, deviation {dev_:.3e}, bound {bound:.3e}')
    assert dev_ <= bound
    m = None if mask is None else S.random_mask(shape, 5, bool if mask == 'bool' else np.uint8)
    isum, fsum = R.residual_nll_finalize(mean, count, dev(m if m is None else m.reshape(shape)))
    wi, wf = S.reference_nll_summary(got_mean, got_count, m)
    assert isum.tolist() == wi and fsum[1].item() == wf[1] and wi[0] > 0
    assert abs(fsum[0].item() - wf[0]) <= SUM_MARGIN * wi[0] * 2.0 ** -53 * float(np.abs(got_mean).sum())
    # nothing under the mask: the maximum nothing entered is -inf
    isum, fsum = R.residual_nll_finalize(mean, count, torch.zeros(shape, device=DEV, dtype=torch.bool))
    assert isum.tolist() == [0, 0] and fsum.tolist() == [0.0, -math.inf]


# ---------------------------------------------------------------- statistical sense
def test_the_right_mixture_fits_and_the_wrong_one_does_not():
    """2 n KL is chi-square with B - 1 degrees of freedom under the model: its mean is B - 1, the bound five times that"""
    B, h = 32, float(np.float32(0.8))  # the float32 the kernel bins with: calc_residual_check fits over the same edges
    z = S.draw_mixture(BIG, 1, STD, PI, seed=7)
    out = R.residual_histogram(dev(z), None, h, B)
    n = int(out['counts'][0, 0])
    right = R.residual_fit(out['hist'], out['counts'], out['sums'], h, STD, PI)[0]
    wrong = R.residual_fit(out['hist'], out['counts'], out['sums'], h, [2 * s for s in STD], PI)[0]
    print(f'n = {n}: KL {right["kl"]:.3e} (bound {5 * (B - 1) / (2 * n):.3e}); doubled scales {wrong["kl"]:.3e}')
    assert n == z.size and right['kl'] < 5 * (B - 1) / (2 * n) and wrong['kl'] > 0.1

    class Model:  # what mixture_terms reads of a GMM
        log_std = torch.log(torch.tensor(STD, dtype=torch.float64))
        log_proportions = torch.log(torch.tensor(PI, dtype=torch.float64))
    rows = calc_residual_check(dev(z), None, Model(), h, B)
    assert rows[0]['kl'] == pytest.approx(right['kl'], rel=1e-9) and rows[0]['n_clipped'] == int(out['counts'][0, 2])


# ---------------------------------------------------------------- the C ABI refuses what it cannot do
def test_abi_refusals():
    lib = L.load()
    shape = (4, 4, 4)
    z = torch.zeros(2, 1, *shape, device=DEV)
    hist = torch.full((2, 8), 7, device=DEV, dtype=torch.int64)
    counts = torch.full((2, 3), 7, device=DEV, dtype=torch.int64)
    sums = torch.full((2, 4), 7.0, device=DEV, dtype=torch.float64)
    mean, count = torch.full(shape, 7.0, device=DEV), torch.full(shape, 7, device=DEV, dtype=torch.int32)
    ws = torch.empty(L.IRS_RESIDUAL_WS_BYTES, device=DEV, dtype=torch.uint8)
    p = lambda t: C.c_void_p(t.data_ptr())

    def histogram(Cn=2, h=0.5, bins=8, before=0, ws_bytes=L.IRS_RESIDUAL_WS_BYTES, dims=shape):
        return lib.irs_residual_histogram(p(z), Cn, None, *dims, h, bins, p(hist), p(counts), p(sums), before, p(ws), ws_bytes, None)

    def update(Cn=2, lw=(0.0,), inv=(1.0,), K=None, before=0):
        K = len(lw) if K is None else K
        arr = C.c_double * max(len(lw), 1)
        return lib.irs_residual_nll_update(p(z), Cn, *shape, arr(*lw), arr(*inv), K, p(mean), p(count), before, None)

    def finalize(ws_bytes):
        isum, fsum = torch.full((2,), 7, device=DEV, dtype=torch.int64), torch.full((2,), 7.0, device=DEV, dtype=torch.float64)
        rc = lib.irs_residual_nll_finalize(p(mean), p(count), None, *shape, p(isum), p(fsum), p(ws), ws_bytes, None)
        assert isum.tolist() == [7, 7] and fsum.tolist() == [7.0, 7.0]
        return rc

    cases = [(lambda: histogram(Cn=0), 'irs_residual_histogram: C = 0 chains, 1..8'),
             (lambda: histogram(Cn=9), 'irs_residual_histogram: C = 9 chains, 1..8'),
             (lambda: histogram(bins=1), 'irs_residual_histogram: bins = 1, 2..512'),
             (lambda: histogram(bins=513), 'irs_residual_histogram: bins = 513, 2..512'),
             (lambda: histogram(h=0.0), 'irs_residual_histogram: half_range = 0, a finite value > 0 needed'),
             (lambda: histogram(h=-1.0), 'irs_residual_histogram: half_range = -1, a finite value > 0 needed'),
             (lambda: histogram(h=math.nan), 'irs_residual_histogram: half_range = nan, a finite value > 0 needed'),
             (lambda: histogram(h=math.inf), 'irs_residual_histogram: half_range = inf, a finite value > 0 needed'),
             (lambda: histogram(h=1e-44), 'irs_residual_histogram: half_range = 9.80909e-45 is too wide or too narrow for float32 bins'),
             (lambda: histogram(dims=(0, 4, 4)), 'irs_residual_histogram: dims (0, 4, 4), every one >= 1 needed'),
             (lambda: histogram(before=-1), 'irs_residual_histogram: records_before = -1 < 0'),
             (lambda: histogram(ws_bytes=L.IRS_RESIDUAL_WS_BYTES - 1),
              f'irs_residual_histogram: workspace of {L.IRS_RESIDUAL_WS_BYTES - 1} bytes, {L.IRS_RESIDUAL_WS_BYTES} needed '
              f'(IRS_RESIDUAL_WS_BYTES)'),
             (lambda: update(Cn=0), 'irs_residual_nll_update: C = 0 chains, 1..8'),
             (lambda: update(K=0), 'irs_residual_nll_update: K = 0 components, 1..8'),
             (lambda: update(lw=(0.0,) * 9, inv=(1.0,) * 9), 'irs_residual_nll_update: K = 9 components, 1..8'),
             (lambda: update(lw=(0.0, math.inf), inv=(1.0, 1.0)), 'irs_residual_nll_update: log_weight[1] = inf, a finite value needed'),
             (lambda: update(lw=(math.nan,)), 'irs_residual_nll_update: log_weight[0] = nan, a finite value needed'),
             (lambda: update(inv=(0.0,)), 'irs_residual_nll_update: inv_std[0] = 0, a finite value > 0 needed'),
             (lambda: update(inv=(math.inf,)), 'irs_residual_nll_update: inv_std[0] = inf, a finite value > 0 needed'),
             (lambda: update(before=-2), 'irs_residual_nll_update: records_before = -2 < 0'),
             (lambda: finalize(L.IRS_RESIDUAL_MAP_WS_BYTES - 1),
              f'irs_residual_nll_finalize: workspace of {L.IRS_RESIDUAL_MAP_WS_BYTES - 1} bytes, {L.IRS_RESIDUAL_MAP_WS_BYTES} needed '
              f'(IRS_RESIDUAL_MAP_WS_BYTES)')]
    for call, message in cases:
        assert call() != 0 and lib.irs_last_error().decode() == message, (lib.irs_last_error().decode(), message)
    torch.cuda.synchronize()
    for t in (hist, counts, count):  # nothing was written
        assert (t == 7).all()
    assert (sums == 7.0).all() and (mean == 7.0).all()


# ---------------------------------------------------------------- the trainer
def make_trainer(tmp_path, dims, **trainer_over):
    from ir_sgmcmc_amd.parse_config import ConfigParser
    from ir_sgmcmc_amd.trainer import Trainer
    cfg = json.load(open(os.path.join(ROOT, 'configs', 'synthetic_gmm_lognormal.json')))
    cfg['trainer']['save_dir'] = str(tmp_path)
    cfg['data_loader']['args']['dims'] = list(dims)
    cfg['trainer'].update(trainer_over)
    config = ConfigParser.from_dict(copy.deepcopy(cfg), timestamp='t')
    dl = config.init_data_loader()
    losses = config.init_losses()
    tm, rm = config.init_transformation_and_registration_modules()
    return Trainer(config, dl, losses, tm, rm, config.init_metrics(), device=DEV)


def test_trainer_vi_stage_logs_the_sample_it_has(tmp_path):
    """two VI iterations with the option on: VI/residuals/* at the logged iterations, nothing accumulated, no MCMC state"""
    from ir_sgmcmc_amd.diagnostics import RESIDUAL_METRICS
    t = make_trainer(tmp_path, (16, 16, 16), VI=True, no_iters_VI=2, no_samples_VI_test=1, log_period_VI=1, MCMC=False,
                     residual_check={'bins': 32, 'nll_map': False})
    t.run()
    res = t.metrics.result()
    for prefix, updates in (('VI/train/residuals', 1), ('VI/residuals', 2)):
        for k, _ in RESIDUAL_METRICS:
            assert t.metrics._count[f'{prefix}/{k}'] == updates and math.isfinite(res[f'{prefix}/{k}']), (prefix, k)
    assert set(t.residual_summary) == {'unregistered'} and t._residual_check is None
    assert 0.0 <= res['VI/residuals/TV'] <= 1.0 and 0.0 <= res['VI/residuals/KS'] <= 1.0


def test_trainer_residual_check(tmp_path):
    from ir_sgmcmc_amd.diagnostics import recorded_steps, residual_check_metric_names
    from ir_sgmcmc_amd.utils.imageio import read_nifti
    N = 16
    kw = dict(no_chains=2, no_iters_burn_in=2, no_samples_MCMC=8, log_period_MCMC=4, checkpoint_period=6)
    on_kw = dict(kw, residual_check={'bins': 64, 'period': 1})
    torch.manual_seed(0)
    a = make_trainer(tmp_path / 'a', (N, N, N), **on_kw)
    a.run()
    C = a.no_chains
    res = a.metrics.result()
    new = residual_check_metric_names(a.residual_options, C)
    assert len(new) == 7 * (C + 2) + 2
    for k in new:
        assert a.metrics._count[k] > 0 and math.isfinite(res[k]), (k, res[k])
    s = a.residual_summary
    assert set(s) == {'unregistered', 'posterior'}
    fixed, _, _ = next(iter(a.data_loader))
    mask = fixed['mask'].reshape(N, N, N) != 0
    post, rc = s['posterior'], a._residual_check
    assert s['unregistered']['n'] + s['unregistered']['n_nonfinite'] == int(mask.sum())
    assert post['records'] == C * len(recorded_steps(2, 8, 1)) == rc.records
    assert post['fit']['n'] + post['n_nonfinite'] == post['records'] * int(mask.sum()) == int(rc.counts[:, :2].sum())
    assert post['half_range'] == a._residual_range == rc.half_range and post['bins'] == 64
    assert post['nll']['voxels'] == int(mask.sum()) and post['nll']['nll_mean'] == res['MCMC/residuals/nll_mean']
    assert post['nll']['nll_mean'] <= post['nll']['nll_max'] == res['MCMC/residuals/nll_max']
    assert int(rc.count.max()) == post['records']
    folder = a.config.save_dirs['samples']
    lines = open(folder / 'MCMC_residual_hist.csv').read().splitlines()
    assert lines[0] == 'bin_lo,bin_hi,count_chain_0,count_chain_1,count,model_probability' and len(lines) == 65
    table = np.array([[float(x) for x in line.split(',')] for line in lines[1:]])
    assert table[:, 4].sum() == post['fit']['n'] and (table[:, 2:4] == rc.hist.cpu().numpy().T).all()
    # the model's proportions come out of a float32 log_softmax: they sum to 1 within a few 2^-24, and so do the bins
    assert table[0, 0] == -rc.half_range and table[-1, 1] == rc.half_range and abs(table[:, 5].sum() - 1.0) < 1e-6
    im = torch.nan_to_num(a.residual_nll_mean.cpu(), nan=0.0).numpy()
    plain, _ = read_nifti(str(folder / 'MCMC_nll_mean.nii.gz'))
    masked, _ = read_nifti(str(folder / 'MCMC_nll_mean_masked.nii.gz'))
    m = mask.numpy()
    assert (plain == im).all() and (masked[m] == im[m]).all() and not masked[~m].any()
    # resumed from the checkpoint in the middle of the recording, the state comes out bit for bit
    ck = a.config.save_dirs['checkpoints'] / 'checkpoint_0000006.pt'
    sd = torch.load(ck, map_location='cpu', weights_only=True)
    assert sd['residual_check']['records'] == C * 4 and sd['residual_check']['half_range'] == rc.half_range
    torch.manual_seed(0)
    b = make_trainer(tmp_path / 'b', (N, N, N), resume=str(ck), **on_kw)
    b.run()
    for name in ('hist', 'counts', 'count'):
        assert torch.equal(getattr(rc, name), getattr(b._residual_check, name)), name
    assert torch.equal(rc.mean.view(torch.int32), b._residual_check.mean.view(torch.int32))
    assert torch.equal(rc.sums.view(torch.int64), b._residual_check.sums.view(torch.int64))
    assert torch.equal(a.v_curr_state.view(torch.int32), b.v_curr_state.view(torch.int32))
    # with the option absent: the same chain and the same metric keys as a run that never heard of the feature
    torch.manual_seed(0)
    off = make_trainer(tmp_path / 'off', (N, N, N), **kw)
    off.run()
    assert off.residual_summary is None and off._residual_check is None
    assert set(off.metrics.result()) == set(res) - set(new)
    assert torch.equal(a.v_curr_state.view(torch.int32), off.v_curr_state.view(torch.int32))
    assert not (off.config.save_dirs['samples'] / 'MCMC_residual_hist.csv').exists()
