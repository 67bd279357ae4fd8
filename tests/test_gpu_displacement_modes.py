"""Posterior principal modes on the GPU ("Displacement modes"): the Gram matrix of the device store bit for bit
on exact cases and within the derived bound on random ones, the projection bit for bit against the restatement's operation order
and its explained ratio within the forward bound, planted modes end to end, every refusal of the C ABI, and the trainer option.
tests/_displacement_modes.py has the restatement and derives every bound.

Figures printed by the bounded comparisons (worst error over bound) are recorded in DESIGN.md.
"""
import copy
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

from ir_sgmcmc_amd import _lib as L
from ir_sgmcmc_amd import modes
from ir_sgmcmc_amd.diagnostics import MODES_METRICS, DisplacementModes, voxel_scale
from ir_sgmcmc_amd.parse_config import ConfigParser
from ir_sgmcmc_amd.trainer import Trainer
from ir_sgmcmc_amd.utils import calc_displacement_modes
from tests import _displacement_modes as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def to_dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # a copy: the shared cases are read-only


def feed(records, appends, mask, cap=None):
    """a fresh state fed `records` in appends of the given sizes -> state"""
    shape = records.shape[2:]
    st = modes.modes_state(shape, sum(appends) if cap is None else cap, DEV, None if mask is None else to_dev(mask))
    x, at = to_dev(records), 0
    for c in appends:
        modes.modes_append(st, x[at:at + c].contiguous())
        at += c
    return st


@pytest.mark.parametrize('family', ['dyadic', 'random'])
@pytest.mark.parametrize('index', range(len(R.GRAM_CASES)))
def test_gram_matrix(index, family):
    shape, appends, kind = R.GRAM_CASES[index]
    records, mask, ref, bound = R.gram_case(index, family)
    st = feed(records, appends, mask)
    n = sum(appends)
    assert st['n'] == n == st['store'].shape[0]  # the last append ended exactly at the cap
    assert st['mask_voxels'] == (int(np.prod(shape)) if mask is None else int(mask.sum()))
    G = modes.modes_gram(st)
    assert G.shape == (3, n, n) and G.dtype == np.float64
    assert np.array_equal(G, np.transpose(G, (0, 2, 1)))  # both triangles from one value
    err = np.abs(G - ref)
    if family == 'dyadic':
        assert np.array_equal(G, ref)
    else:
        with np.errstate(invalid='ignore', divide='ignore'):
            ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
        print({'gram: worst error': float(err.max()), 'worst error / bound': float(ratio.max())})
        assert (err <= bound).all()
    if kind == 'empty':
        assert not G.any()
    # repeatability: a second fresh state, fed in other portions, holds the same bits (the order of a sum does not depend on n)
    other = feed(records, (1,) * n, mask)
    assert torch.equal(other['gram'].view(torch.int64), st['gram'].view(torch.int64))


def test_gram_ignores_what_the_mask_leaves_out_and_propagates_what_it_admits():
    shape = (5, 6, 7)
    records = R.random_records(4, shape, 3).copy()
    mask = R.make_mask('random', shape)
    outside = tuple(np.argwhere(~mask)[0])
    inside = tuple(np.argwhere(mask)[0])
    clean = modes.modes_gram(feed(records, (2, 2), mask))
    records[1][(0,) + outside] = np.nan
    records[2][(1,) + outside] = np.inf
    assert np.array_equal(modes.modes_gram(feed(records, (2, 2), mask)), clean)
    records[3][(2,) + inside] = np.nan
    G = modes.modes_gram(feed(records, (2, 2), mask))
    assert np.isnan(G[2, 3]).all() and np.isnan(G[2, :, 3]).all() and np.array_equal(G[:2], clean[:2])
    assert np.array_equal(G[2, :3, :3], clean[2, :3, :3])


def test_appending_after_a_state_dict_round_trip_is_bit_identical():
    shape = (5, 6, 7)
    records = to_dev(R.random_records(9, shape, 11))
    mask = to_dev(R.make_mask('random', shape))
    a = DisplacementModes(shape, DEV, 12, mask)
    b = DisplacementModes(shape, DEV, 12, mask)
    for lo, hi in ((0, 2), (2, 5)):
        a.record(records[lo:hi].contiguous())
        b.record(records[lo:hi].contiguous())
    sd = copy.deepcopy(b.state_dict())
    assert sd['records'] == 5 and tuple(sd['store'].shape) == (5, 3) + shape and sd['chains'] == [0, 1, 0, 1, 2]
    c = DisplacementModes(shape, DEV, 12, mask)
    c.load_state_dict(sd)
    for lo, hi in ((5, 8), (8, 9)):
        a.record(records[lo:hi].contiguous())
        c.record(records[lo:hi].contiguous())
    assert torch.equal(a.dev['gram'].view(torch.int64), c.dev['gram'].view(torch.int64))
    assert torch.equal(a.dev['store'][:9], c.dev['store'][:9]) and a.steps == c.steps and a.chains == c.chains
    fa, fc = a.finalize(3), c.finalize(3)
    assert np.array_equal(fa['eigenvalues'], fc['eigenvalues']) and torch.equal(fa['modes'], fc['modes'])
    with pytest.raises(ValueError, match='do not match'):
        DisplacementModes((5, 6, 8), DEV, 12).load_state_dict(sd)
    with pytest.raises(ValueError, match='max_records'):
        DisplacementModes(shape, DEV, 13).load_state_dict(sd)
    with pytest.raises(ValueError, match='exceed the store'):
        a.record(records[:4].contiguous())


@pytest.mark.parametrize('n,M,recipe', R.PROJECT_CASES)
@pytest.mark.parametrize('shape', R.SHAPES)
def test_projection(shape, n, M, recipe):
    records, coeff, scale, want, ref = R.project_case(shape, n, M, recipe)
    st = feed(records, (n,) if n <= 8 else (8,) * (n // 8), None)
    mean, fields, explained = modes.modes_project(st, coeff, scale)
    assert mean.dtype == fields.dtype == explained.dtype == torch.float32 and tuple(fields.shape) == (M, 3) + shape
    assert np.array_equal(mean.cpu().numpy().view(np.int32), want['mean'].view(np.int32))
    assert np.array_equal(fields.cpu().numpy().view(np.int32), want['modes'].view(np.int32))
    R.check_explained(explained.cpu().numpy(), ref)
    if n == 1:
        assert not explained.any()


def test_projection_of_volumes_with_rows_that_never_move():
    """rows of zeros and rows of one small dyadic constant: every intermediate is exact there, the denominator is exactly 0 and
    the explained ratio exactly 0; a NaN propagates to its own voxel only"""
    shape, n, M = (5, 6, 7), 7, 3
    records = R.random_records(n, shape, 21).copy()
    records[:, :, 0] = 0.0
    records[:, :, 1] = np.float32(0.1875)
    records[3, 1, 4, 2, 5] = np.nan
    coeff = np.random.default_rng(2).standard_normal((M, n))
    scale = R.default_scale(shape)
    mean, fields, explained = modes.modes_project(feed(records, (n,), None), coeff, scale)
    want = R.project_np(records, coeff, scale)
    e = explained.cpu().numpy()
    assert not e[:2].any() and np.isnan(e[4, 2, 5]) and np.isfinite(np.delete(e.reshape(-1), (4 * 6 + 2) * 7 + 5)).all()
    assert np.array_equal(mean.cpu().numpy().view(np.int32), want['mean'].view(np.int32))
    assert np.array_equal(fields.cpu().numpy().view(np.int32), want['modes'].view(np.int32))
    assert np.array_equal(e.view(np.int32)[:2], want['explained'].view(np.int32)[:2])
    assert float(mean[1, 1].min()) == float(mean[1, 1].max()) == 0.1875


@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('n,Cn', R.PLANTED_CASES)
def test_planted_modes_end_to_end(n, Cn, masked):
    shape = (16, 12, 20)
    mask = R.make_mask('random', shape) if masked else None
    records, psi, scale = R.planted_records(n, shape, 100 * n + Cn, mask)
    assert n % Cn == 0
    out = calc_displacement_modes(to_dev(records), None if mask is None else to_dev(mask), 3, chains=Cn)
    lam, s = out['eigenvalues'], out['summary']
    a2 = np.asarray(R.AMPLITUDES) ** 2
    # the inputs: the sample eigenvalues sit at 16 : 4 : 1 with every relative gap >= 0.5, no mode left out
    gaps = (lam[:3] - np.append(lam[1:3], lam[3] if len(lam) > 3 else 0.0)) / lam[:3]
    assert (gaps >= 0.5).all(), gaps
    # Weyl, from the Gram bound and the noise
    _, bound = R.gram_reference(records, mask)
    s2 = np.asarray(scale).reshape(3, 1, 1) ** 2
    eG = float(np.sqrt((((s2 * bound).sum(axis=0)) ** 2).sum())) / (n - 1)
    N2 = R.planted_perturbation(records, psi, scale, mask)
    err = np.abs(lam[:3] - a2)
    print({'planted eigenvalues: worst error / bound': float((err / (N2 + eG)).max()), 'N2': N2, 'eG': eG})
    assert (err <= N2 + eG).all()
    # Davis-Kahan for each of the three mode fields, in the masked, scaled inner product
    levels = np.append(a2, 0.0)
    fields = out['modes'].cpu().numpy().astype(np.float64).reshape(3, 3, -1) * np.asarray(scale).reshape(1, 3, 1)
    if mask is not None:
        fields = fields * mask.reshape(1, 1, -1)
    fields = fields.reshape(3, -1)
    worst = 0.0
    for m in range(3):
        delta = min(abs(levels[m] - levels[k]) for k in range(4) if k != m)
        phi = fields[m] / np.linalg.norm(fields[m])
        cos = abs(float(phi @ psi[m]))
        sin = math.sqrt(max(0.0, 1.0 - cos * cos))
        tol = 2 * (N2 + eG) / delta + 2.0 ** -20
        worst = max(worst, sin / tol)
        assert sin <= tol, (m, sin, tol)
        # the norm of a 1-sigma mode is sqrt(lambda_m)
        assert abs(np.linalg.norm(fields[m]) - math.sqrt(lam[m])) <= 2.0 ** -20 * math.sqrt(lam[m])
    print({'planted modes: worst sine / bound': worst})
    support = (psi.reshape(3, 3, -1) != 0).any(axis=(0, 1)).reshape(shape)
    assert float(out['explained_map'][to_dev(support)].min()) >= 0.99
    assert s['n90'] <= 2 and s['records'] == n and s['modes'] == 3
    assert math.isnan(s['rhat_max']) == (Cn < 2 or n // Cn < 4)
    assert out['chains'] == list(range(Cn)) * (n // Cn)


def test_abi_refusals_and_the_workspace_query():
    lib = L.load()
    D, H, W, cap = 4, 5, 6, 6
    store = torch.zeros(cap, 3, D, H, W, device=DEV)
    gram = torch.zeros(3, cap, cap, device=DEV, dtype=torch.float64)
    need = C.c_size_t()
    L.check(lib.irs_modes_gram_workspace(D, H, W, 2, C.byref(need)))
    more = C.c_size_t()
    L.check(lib.irs_modes_gram_workspace(D, H, W, 8, C.byref(more)))
    assert 0 < need.value < more.value and more.value == 4 * need.value and need.value % 8 == 0
    ws = torch.empty(need.value, device=DEV, dtype=torch.uint8)
    coeff = torch.zeros(2, 3, device=DEV, dtype=torch.float64)
    mean, fields, ex = torch.empty(3, D, H, W, device=DEV), torch.empty(2, 3, D, H, W, device=DEV), torch.empty(D, H, W, device=DEV)
    q = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    st = L.stream_ptr()
    good = (C.c_double * 3)(1.0, 1.0, 1.0)

    def refused(rc, text):
        assert rc != 0
        msg = lib.irs_last_error().decode()
        assert text in msg, msg

    def query(D_=D, n_new=2, out=C.byref(need)):
        return lib.irs_modes_gram_workspace(D_, H, W, n_new, out)

    def rows(store_=store, cap_=cap, before=0, n_new=2, D_=D, gram_=gram, ws_=ws, ws_bytes=None):
        return lib.irs_modes_gram_rows(q(store_), cap_, before, n_new, D_, H, W, None, q(gram_), q(ws_),
                                       need.value if ws_bytes is None else ws_bytes, st)

    def project(store_=store, n=3, D_=D, coeff_=coeff, M=2, scale=good, mean_=mean, fields_=fields, ex_=ex):
        return lib.irs_modes_project(q(store_), n, D_, H, W, q(coeff_), M, scale, q(mean_), q(fields_), q(ex_), st)

    refused(query(out=None), 'irs_modes_gram_workspace: null pointer')
    refused(query(D_=0), 'irs_modes_gram_workspace: dims (0, 5, 6), every one >= 1 needed')
    refused(query(n_new=0), 'irs_modes_gram_workspace: n_new = 0 records, 1..8')
    refused(query(n_new=9), 'irs_modes_gram_workspace: n_new = 9 records, 1..8')
    for kw in (dict(store_=None), dict(gram_=None), dict(ws_=None)):
        refused(rows(**kw), 'irs_modes_gram_rows: null pointer')
    refused(rows(cap_=0), 'irs_modes_gram_rows: cap = 0 records, 1..1024')
    refused(rows(cap_=1025), 'irs_modes_gram_rows: cap = 1025 records, 1..1024')
    refused(rows(n_new=0), 'irs_modes_gram_rows: n_new = 0 records, 1..8')
    refused(rows(n_new=9), 'irs_modes_gram_rows: n_new = 9 records, 1..8')
    refused(rows(before=-1), 'irs_modes_gram_rows: records_before = -1 < 0')
    refused(rows(before=5), "irs_modes_gram_rows: 5 records + 2 chains exceed the store's cap")
    refused(rows(D_=0), 'irs_modes_gram_rows: dims (0, 5, 6), every one >= 1 needed')
    refused(rows(ws_bytes=need.value - 8), 'irs_modes_gram_workspace')
    for kw in (dict(store_=None), dict(coeff_=None), dict(scale=None), dict(mean_=None), dict(fields_=None), dict(ex_=None)):
        refused(project(**kw), 'irs_modes_project: null pointer')
    refused(project(n=0), 'irs_modes_project: n = 0 records, 1..1024')
    refused(project(M=0), 'irs_modes_project: M = 0 modes, 1..16')
    refused(project(M=17), 'irs_modes_project: M = 17 modes, 1..16')
    refused(project(D_=-1), 'irs_modes_project: dims (-1, 5, 6), every one >= 1 needed')
    for bad in ((0.0, 1, 1), (1, -2.0, 1), (1, 1, float('nan')), (float('inf'), 1, 1)):
        refused(project(scale=(C.c_double * 3)(*bad)), 'a finite value > 0 needed')
    torch.cuda.synchronize()
    assert not gram.any()  # nothing was written by a refused call
    L.check(rows())
    L.check(project())
    torch.cuda.synchronize()
    # the Python surface
    state = modes.modes_state((D, H, W), cap, DEV)
    x = torch.zeros(2, 3, D, H, W, device=DEV)
    for bad in (lambda: modes.modes_state((D, H, W), 0, DEV), lambda: modes.modes_state((D, H, W), 1025, DEV),
                lambda: modes.modes_state((D, H), 4, DEV), lambda: modes.modes_append(state, x.cpu()),
                lambda: modes.modes_append(state, x.double()), lambda: modes.modes_append(state, x[:, :2].contiguous()),
                lambda: modes.modes_append(state, torch.zeros(9, 3, D, H, W, device=DEV)),
                lambda: modes.modes_state((D, H, W), 4, DEV, mask=torch.ones(D, H, W, device=DEV)),
                lambda: modes.modes_project(state, np.zeros((2, 3)), (1, 1, 1))):
        with pytest.raises(L.IrsError):
            bad()


# ---------------------------------------------------------------- the trainer option
def make_trainer(tmp_path, dims, **trainer_over):
    cfg = json.load(open(os.path.join(ROOT, 'configs', 'synthetic_ssd_l2_128_modes.json')))
    cfg['trainer']['save_dir'] = str(tmp_path)
    cfg['data_loader']['args']['dims'] = list(dims)
    for key in ('displacement_modes', 'displacement_covariance', 'convergence_diagnostics'):
        cfg['trainer'].pop(key)
    cfg['trainer'].update(trainer_over)
    config = ConfigParser.from_dict(copy.deepcopy(cfg), timestamp='t')
    dl = config.init_data_loader()
    losses = config.init_losses()
    tm, rm = config.init_transformation_and_registration_modules()
    return Trainer(config, dl, losses, tm, rm, config.init_metrics(), device=DEV)


NEW_FILES = ['MCMC_mode_1.vtk', 'MCMC_mode_2.vtk', 'MCMC_mode_3.vtk', 'MCMC_mode_scores.csv', 'MCMC_modes.csv',
             'MCMC_modes_explained.nii.gz', 'MCMC_modes_explained_masked.nii.gz']


def _file_bytes(trainer):
    """every file of the samples folder, the gzipped ones unpacked (a gzip header carries the time it was written)"""
    import gzip
    folder = trainer.config.save_dirs['samples']
    return {p.name: gzip.decompress(p.read_bytes()) if p.name.endswith('.gz') else p.read_bytes()
            for p in folder.iterdir() if p.is_file()}


def test_trainer_option_changes_nothing_else_and_writes_its_outputs(tmp_path):
    N = 32
    kw = dict(no_chains=2, no_iters_burn_in=4, no_samples_MCMC=8, log_period_MCMC=2)
    torch.manual_seed(0)
    on = make_trainer(tmp_path / 'on', (N, N, N), displacement_modes={'modes': 3, 'max_records': 8},
                      displacement_covariance=True, **kw)
    on.run()
    torch.manual_seed(0)
    off = make_trainer(tmp_path / 'off', (N, N, N), displacement_covariance=True, **kw)
    off.run()
    assert torch.equal(on.v_curr_state, off.v_curr_state)
    assert torch.equal(on.displacement_mean, off.displacement_mean) and torch.equal(on.displacement_std, off.displacement_std)
    files_on, files_off = _file_bytes(on), _file_bytes(off)
    assert sorted(files_on) == sorted(list(files_off) + NEW_FILES)
    assert all(files_on[name] == data for name, data in files_off.items())
    assert off.displacement_modes_summary is None and off.displacement_mode_fields is None and off._displacement_modes is None
    res, res_off = on.metrics.result(), off.metrics.result()
    assert [k for k in res if k.startswith('MCMC/modes/')] == [f'MCMC/modes/{k}' for k in MODES_METRICS]
    assert [k for k in res if not k.startswith('MCMC/modes/')] == list(res_off)
    i = list(res).index('MCMC/modes/var_total')
    assert list(res)[i - 1].startswith('MCMC/covariance/')  # after the covariance keys
    s = on.displacement_modes_summary
    for k in MODES_METRICS:
        got = res[f'MCMC/modes/{k}']
        assert (math.isnan(got) and math.isnan(s[k])) or got == s[k]
    assert s['records'] == 8 and s['modes'] == 3 and tuple(on.displacement_mode_fields.shape) == (3, 3, N, N, N)
    assert on.displacement_mode_scores.shape == (8, 3) and on._displacement_modes.steps == [6, 6, 8, 8, 10, 10, 12, 12]
    lines = (on.config.save_dirs['samples'] / 'MCMC_modes.csv').read_text().splitlines()
    assert lines[0] == 'm,eigenvalue,share,cumulative_share,rhat' and len(lines) == 4
    lines = (on.config.save_dirs['samples'] / 'MCMC_mode_scores.csv').read_text().splitlines()
    assert lines[0] == 'record,step,chain,score_1,score_2,score_3' and len(lines) == 9 and lines[4].startswith('3,8,1,')
    # var_total against the covariance state of the same records: sum over the mask of trace S(x).  Both are exact functions of
    # the same float32 records but for rounding: the covariance row's float32 Welford state within FACTOR dM_aa per voxel (its
    # own state bound), the Gram route within gamma_k sum |x_i x_j| per entry, far below it.
    from tests._displacement_covariance import FACTOR as COV_FACTOR, covariance_np
    dm = on._displacement_modes
    records = dm.dev['store'][:8].cpu().numpy()
    mask = dm.dev['mask'].cpu().numpy() != 0
    ref = covariance_np(records, mask=mask)
    scale = voxel_scale((N, N, N))
    com = on._displacement_covariance.comoment[:3].cpu().numpy().astype(np.float64)
    trace = sum(scale[a] ** 2 * com[a][mask].sum() for a in range(3)) / 7
    tol = sum(scale[a] ** 2 * (COV_FACTOR * ref['dM'][a][mask]).sum() for a in range(3)) / 7
    print({'var_total against the covariance state': (abs(trace - s['var_total']), abs(trace - s['var_total']) / tol)})
    assert abs(trace - s['var_total']) <= tol


def test_trainer_modes_survive_checkpoint_resume_bit_for_bit(tmp_path):
    kw = dict(no_chains=2, no_iters_burn_in=2, no_samples_MCMC=8, log_period_MCMC=4, checkpoint_period=6,
              displacement_modes={'period': 2, 'modes': 4, 'max_records': 8}, save_outputs=False)
    a = make_trainer(tmp_path / 'a', (16, 16, 16), **kw)
    a.run()
    ck = a.config.save_dirs['checkpoints'] / 'checkpoint_0000006.pt'
    sd = torch.load(ck, map_location='cpu', weights_only=True)
    assert sd['displacement_modes']['records'] == 4 and tuple(sd['displacement_modes']['store'].shape) == (4, 3, 16, 16, 16)
    b = make_trainer(tmp_path / 'b', (16, 16, 16), resume=str(ck), **kw)
    b.run()
    assert torch.equal(a._displacement_modes.dev['gram'].view(torch.int64), b._displacement_modes.dev['gram'].view(torch.int64))
    assert torch.equal(a.displacement_mode_fields.view(torch.int32), b.displacement_mode_fields.view(torch.int32))
    assert np.array_equal(a.displacement_mode_scores, b.displacement_mode_scores)
    assert json.dumps(a.displacement_modes_summary, sort_keys=True) == json.dumps(b.displacement_modes_summary, sort_keys=True)
    del sd['displacement_modes']
    ck2 = tmp_path / 'no_modes.pt'
    torch.save(sd, ck2)
    c = make_trainer(tmp_path / 'c', (16, 16, 16), resume=str(ck2), **kw)
    with pytest.raises(ValueError, match='displacement_modes'):
        c.run()
