"""Host side of tests/test_gpu_data_gradient.py: the float64 restatement of the data-gradient stage (tests/_data_gradient.py) against the
CPU oracle run in float64 at velocity zero (which pins the constant of the read-out and the face zeros), the same formulas in float32
against the tolerance (a quarter of it at the most), the proof that the tolerance sees the mistakes it is for (each beaten 10x at its
worst element by a deliberate mistake in a copy of the restatement; the measured ratios are in DESIGN.md), and the conditions every
case of the GPU test has to meet for that to mean something -- the cases of the list-walking kernels (G.SPARSE_CASES) included: their
masks leave planes out of every list's reach, and a reach one short or a missing fill there is beyond the tolerance."""
import pytest
import torch

from oracle import OracleChain, OracleConfig
from tests import _data_gradient as G
from tests import _transition_scalars as R

F64 = torch.float64
A, B, E, M = G.DYADIC


def hyper(K, kw):
    return R.Hyper(K=K, data_loss=kw.get('data_loss', 'GMM'), virtual_decimation=kw.get('virtual_decimation', True), conc=[0.5] * K)


# ------------------------------------------------------------------------------------------------------------------------------
# a. the restatement is the oracle transition in float64
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('vd', [True, False])
@pytest.mark.parametrize('data_loss', ['GMM', 'SSD'])
@pytest.mark.parametrize('dims,s', [(A, 1), (A, 2), (B, 2), (E, 1)])
def test_restatement_is_the_oracle_in_float64(dims, s, data_loss, vd):
    C = 2
    fixed, moving, mask = G.case_inputs(dims, C, 'per_chain', True)
    oc = OracleConfig(dims=dims, no_chains=C, sobolev_s=None, uniform_noise=None, lcc_s=s, data_loss=data_loss, virtual_decimation=vd, lr=0.05)
    torch.set_default_dtype(F64)
    try:
        fx, mv = {'im': fixed.to(F64), 'mask': mask}, {'im': moving.to(F64).expand(C, -1, -1, -1, -1).contiguous()}
        orc = OracleChain(oc)
        orc.init_gmm(fx, mv)
        o = orc.transition(fx, mv, torch.zeros(C, 3, *dims))
    finally:
        torch.set_default_dtype(torch.float32)
    assert float(o['displacement'].abs().max()) == 0.0 and float(o['curr_state'].abs().max()) == 0.0
    h = R.Hyper(K=4, data_loss=data_loss, virtual_decimation=vd, ssd_inv_sigma=1.0 / oc.ssd_sigma)
    z, _ = G.forward(fixed, moving, h, s)
    assert float((z - o['residuals']).abs().max()) < 1e-10 * float(z.abs().max())
    params = [(o['gmm_log_std'][c], o['gmm_logits'][c]) for c in range(C)]
    r = G.data_gradient(o['residuals'], moving, fixed, mask, o['alpha'], params, h, s)
    g = o['grad_v']
    assert float((r['grad_v'] - g).abs().max()) < 1e-10 * float(g.abs().max())
    if vd:
        assert all(0.0 < a < 0.9 for a in o['alpha']), o['alpha']
    # channel ch is exactly 0 on both faces of its own axis, in the oracle as in the restatement
    for ch, ax in enumerate((-1, -2, -3)):
        for t in (g, r['grad_v']):
            assert float(t[:, ch].narrow(ax, 0, 1).abs().max()) == 0.0 and float(t[:, ch].narrow(ax, dims[ax] - 1, 1).abs().max()) == 0.0
    # ... and the explicit box^T formulas are the float64 autograd of the restated map
    if data_loss == 'GMM':
        g_z = torch.randn(C, 1, *dims, dtype=F64, generator=torch.Generator().manual_seed(5))
        wh, sigma, _ = G.lcc_stats(moving[0, 0].to(F64), s)
        ref = G.lcc_adjoint_autograd(g_z, fixed, moving.expand(C, -1, -1, -1, -1), s)
        got = torch.stack([G.lcc_adjoint(g_z[c, 0], wh, sigma, s)[0] for c in range(C)]).unsqueeze(1)
        assert float((got - ref).abs().max()) < 1e-12 * float(ref.abs().max())


# ------------------------------------------------------------------------------------------------------------------------------
# the cases of the GPU test, as far as the CPU can form them: the residual from a float32 evaluation of the forward map
# ------------------------------------------------------------------------------------------------------------------------------
_cache = {}


def host_case(case):
    """-> dict: inputs, float32 residual z (C,1,D,H,W), hyper, mixture state, restatement `ref` and records `recs`"""
    key = G.case_id(case)
    if key not in _cache:
        dims, s, C, K, mask_kind, per_chain_fixed, kw = case
        fixed, moving, mask = G.case_inputs(dims, C, mask_kind, per_chain_fixed)
        h = hyper(K, kw)
        z32, tol_z = G.forward(fixed, moving, h, s, torch.float32)
        z64, _ = G.forward(fixed, moving, h, s)
        z32 = z32.expand(C, -1, -1, -1, -1).contiguous()
        state = G.mixture_state(fixed, moving, mask, K, s) if h.data_loss == 'GMM' else None
        ref, recs = G.reference(z32.to(F64), fixed, moving, mask, h, s, state)
        _cache[key] = dict(fixed=fixed, moving=moving, mask=mask, h=h, s=s, C=C, K=K, z32=z32, z64=z64, tol_z=tol_z, state=state, ref=ref, recs=recs,
                           alpha=[r['alpha'] for r in recs], params=[(r['log_std'], r['logits']) for r in recs])
    return _cache[key]


def worst(got, ref, finite=False):
    """largest deviation in units of the tolerance (an exact match counts 0, whatever the tolerance).  finite: elements whose tolerance
    is exactly 0 are left out, so that the ratio is a number -- it can only come out smaller"""
    dev = (got.to(F64) - ref['grad_v']).abs()
    skip = (dev == 0) | (ref['tol'] == 0) if finite else dev == 0
    return float(torch.where(skip, torch.zeros_like(dev), dev / ref['tol']).max())


def wrong(c, **kw):
    """the restatement of host case c with something changed"""
    a = dict(z=c['z32'].to(F64), moving=c['moving'], fixed=c['fixed'], mask=c['mask'], alpha=c['alpha'], params=c['params'], h=c['h'], s=c['s'])
    a.update(kw)
    return G.data_gradient(**a)['grad_v']


# b. float32 on the CPU stays inside a quarter of the tolerance; d. the inputs keep the reference inside the conditions
ALL_CASES = G.ENGINE_CASES + G.SPARSE_CASES


@pytest.mark.parametrize('case', ALL_CASES, ids=[G.case_id(c) for c in ALL_CASES])
def test_every_gpu_case_float32_fits_and_conditions_hold(case):
    dims, s, C, K, mask_kind, per_chain_fixed, kw = case
    c = host_case(case)
    h, ref = c['h'], c['ref']
    gmm = h.data_loss == 'GMM'
    # the forward map in float32 fits ITS tolerance ...
    dz = (c['z32'].to(F64) - c['z64']).abs()
    assert float(torch.where(dz == 0, torch.zeros_like(dz), dz / c['tol_z']).max()) <= 1.0
    # ... and the stage in float32, w / sigma taken as fhat - z like the kernel does, a quarter of the gradient's
    f32 = G.data_gradient(c['z32'], c['moving'], c['fixed'], c['mask'], c['alpha'], c['params'], h, s, dtype=torch.float32, w_from_z=True)
    ratio = worst(f32['grad_v'], ref)
    print(f'float32 / tolerance {ratio:.4f}')
    assert ratio <= 0.25
    assert bool(torch.isfinite(ref['grad_v']).all()) and bool((ref['tol'] >= 0).all())
    # alpha: well below 1 wherever virtual decimation acts (exactly 1 on the checkerboard, whose lag pairs all have a member off the mask)
    for a in c['alpha']:
        if not h.virtual_decimation or mask_kind == 'checkerboard':
            assert a == 1.0
        else:
            assert 0.0 < a < 0.9, c['alpha']
    # several chains: the stepped parameters of consecutive chains differ by at least 100x their tolerance
    if gmm and C > 1:
        for r0, r1 in zip(c['recs'][:-1], c['recs'][1:]):
            d = torch.stack([r1['log_std'] - r0['log_std'], r1['logits'] - r0['logits']]).abs()
            assert bool((d >= 100.0 * torch.maximum(r0['tol_param'], r1['tol_param'])).all()), (d, r1['tol_param'])
    # coverage: every channel non-zero on >= 80 % of the interior voxels.  Two kinds of case cannot reach that by construction and are held
    # to what they can: the two-plane mask reaches 2 + 4 S planes (all of them, >= 80 % of each), and the SSD term is pointwise -- g_M
    # is non-zero exactly on the mask, all of it
    g = ref['grad_v']
    D = dims[0]
    for ch in range(3):
        inner = g[:, ch, 1:-1, 1:-1, 1:-1] != 0
        if not gmm:
            mk = c['mask'].expand(C, -1, -1, -1, -1)[:, 0, 1:-1, 1:-1, 1:-1]
            assert bool((inner == mk).all())
        elif mask_kind == 'seam_planes':
            lo, hi = max(3 - 2 * s, 1), min(4 + 2 * s, D - 2)
            assert float(inner[:, lo - 1:hi].double().mean()) >= 0.8 and not bool(inner[:, hi:].any()) and not bool(inner[:, :lo - 1].any())
        elif mask_kind == 'band':
            # four planes of the synthetic mask reach 4 + 4 S planes: every one of them shows, nothing beyond them does
            lo, hi = max(D // 2 - 2 - 2 * s, 1), min(D // 2 + 1 + 2 * s, D - 2)
            assert bool(inner[:, lo - 1:hi].flatten(2).any(2).all()) and not bool(inner[:, hi:].any()) and not bool(inner[:, :lo - 1].any())
        else:
            assert float(inner.double().mean()) >= 0.8, float(inner.double().mean())
    # the voxels no channel shows are the 8 corners, as a count
    assert G.invisible_voxels(dims) == 8
    assert int(((ref['dm'] != 0).sum(1) == 0).sum()) == 8


# ------------------------------------------------------------------------------------------------------------------------------
# c. deliberate mistakes, each at least 10x the tolerance at its worst element
# ------------------------------------------------------------------------------------------------------------------------------
ONE = (A, 1, 1, 4, 'faces', False, {})
ONE_S2 = (A, 2, 1, 4, 'faces', False, {})
THREE = (A, 1, 3, 4, 'per_chain', True, {})
K5 = (E, 1, 1, 5, 'synthetic', False, {})
K8 = (M, 2, 1, 8, 'synthetic', False, {})
SSD = (A, 1, 2, 1, 'synthetic', False, {'data_loss': 'SSD'})


def seen(name, ratio):
    print(f'mistake: {name}: {ratio:.3g} x tolerance')
    assert ratio >= 10.0, (name, ratio)


@pytest.mark.parametrize('case', [ONE, ONE_S2], ids=['s1', 's2'])
@pytest.mark.parametrize('axis', [-3, -2, -1])
@pytest.mark.parametrize('end', [0, 1])
def test_tolerance_sees_a_dropped_border_weight(case, axis, end):
    c = host_case(case)
    seen(f'box^T border weight dropped, axis {axis} end {end}, S = {c["s"]}', worst(wrong(c, drop={(axis, end)}), c['ref']))


@pytest.mark.parametrize('case', [ONE, ONE_S2], ids=['s1', 's2'])
def test_tolerance_sees_an_unprimed_ring_at_a_seam_and_the_wrong_n(case):
    c = host_case(case)
    seen(f'ring not primed at the seam at plane 4, S = {c["s"]}', worst(wrong(c, seam=4), c['ref']))
    seen(f'1 / n with n = (2S+1)^2, S = {c["s"]}', worst(wrong(c, n=(2 * c['s'] + 1) ** 2), c['ref']))
    seen(f'alpha left out, S = {c["s"]}', worst(wrong(c, alpha=[1.0] * c['C']), c['ref']))


def test_tolerance_sees_a_neighbours_parameters_mask_and_fixed_image():
    c = host_case(THREE)
    st = c['state']
    shifted = [(st['log_std'].to(F64), st['logits'].to(F64))] + c['params'][:-1]
    g = wrong(c, params=shifted)
    for ch in (1, 2):     # chain by chain: the tolerance of chain c includes the spread of ITS parameters
        one = {'grad_v': c['ref']['grad_v'][ch:ch + 1], 'tol': c['ref']['tol'][ch:ch + 1]}
        seen(f'chain {ch} evaluated with the parameters of chain {ch - 1}', worst(g[ch:ch + 1], one))
        # (both also put non-zero values where the reference and its tolerance are exactly 0: left out, to get a number)
        seen(f'chain {ch} with the mask of chain 0', worst(wrong(c, mask=c['mask'][:1])[ch:ch + 1], one, finite=True))
        # (the kernel forms w / sigma as fhat - z: that is where another chain's fixed image enters)
        seen(f'chain {ch} with the fixed image of chain 0', worst(wrong(c, fixed=c['fixed'][:1], w_from_z=True)[ch:ch + 1], one, finite=True))


@pytest.mark.parametrize('case', [K5, K8], ids=['K5', 'K8'])
def test_tolerance_sees_ignored_components_beyond_four(case):
    c = host_case(case)
    seen(f'K = {c["K"]}: components beyond the fourth ignored', worst(wrong(c, params=[(ls[:4], lg[:4]) for ls, lg in c['params']]), c['ref']))


# ------------------------------------------------------------------------------------------------------------------------------
# e. the cases of test_list_kernels_element_by_element: the lists leave planes unmarched, and the tolerance sees what a list-walking
# data stage can get wrong there
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', G.SPARSE_CASES, ids=[G.case_id(c) for c in G.SPARSE_CASES])
def test_sparse_cases_leave_planes_unmarched(case):
    """at reach S (LCC map), 2 S (data term: tile 32 x 16) and 3 S (warp: tile 64 x 8) the run ranges the mask's geometry gives stay
    below D x tile columns, and some run range is longer than two pieces: there are seams inside it"""
    from tests.test_gpu_sparse_data import columns, planes_of, run_lengths
    dims, s, C, K, mask_kind, per_chain_fixed, kw = case
    _, _, mask = G.case_inputs(dims, C, mask_kind, per_chain_fixed)
    assert mask.shape[0] == 1 and mask_kind in ('band', 'seam_planes') and dims in (E, M) and kw.get('data_loss', 'GMM') == 'GMM'
    m3 = mask[0, 0]
    for tile, reach in (((32, 16), s), ((32, 16), 2 * s), ((64, 8), 3 * s)):
        runs = run_lengths(m3, tile, reach)
        assert 0 < planes_of(runs) < dims[0] * columns(dims, tile), (tile, reach, planes_of(runs))
        assert max(b - a for a, b in runs) < dims[0]
    assert max(b - a for a, b in run_lengths(m3, (32, 16), 2 * s)) > G.SPARSE_PIECE
    assert int(G.plane_distance(m3).max()) > 3 * s      # whole planes beyond every reach


def test_sparse_cases_cover_what_they_are_for():
    cases = G.SPARSE_CASES
    assert {(c[1], c[3]) for c in cases} >= {(s, K) for s in (1, 2) for K in (4, 5, 8)}
    assert {c[0] for c in cases} == {E, M} and {c[4] for c in cases} == {'band', 'seam_planes'}
    assert any(c[2] == 3 and c[5] for c in cases) and any(c[2] == 1 for c in cases)
    assert any(c[6].get('virtual_decimation') is False for c in cases) and any('virtual_decimation' not in c[6] for c in cases)
    assert not {G.case_id(c) for c in cases} & {G.case_id(c) for c in G.ENGINE_CASES}


@pytest.mark.parametrize('case', G.SPARSE_CASES, ids=[G.case_id(c) for c in G.SPARSE_CASES])
def test_tolerance_sees_a_short_reach_and_a_missing_fill(case):
    c = host_case(case)
    seen(f'LCC map marched to reach S - 1, S = {c["s"]}', worst(wrong(c, stale_map=c['s'] - 1), c['ref']))
    # (a missing fill leaves values where the reference and its tolerance are exactly 0: any of them is beyond the tolerance)
    g = wrong(c, no_fill=True)
    far = (G.plane_distance(c['mask'][0, 0]) > 2 * c['s']).expand(c['mask'].shape[-3:])
    assert float(c['ref']['grad_v'][..., far].abs().max()) == 0.0 and float(c['ref']['tol'][..., far].max()) == 0.0
    assert float(g[..., far].abs().max()) > 0.0
    seen(f'data term without its zero fill, S = {c["s"]}', worst(g, c['ref']))
    # ... and the mistakes of the dense kernels, where these masks can show them: a seam inside the run range (between two pieces of
    # G.SPARSE_PIECE planes), the wrong 1 / n, alpha left out
    seam = 4 if case[4] == 'seam_planes' else case[0][0] // 2
    seen(f'ring not primed at the seam at plane {seam}, S = {c["s"]}', worst(wrong(c, seam=seam), c['ref']))
    seen(f'1 / n with n = (2S+1)^2, S = {c["s"]}', worst(wrong(c, n=(2 * c['s'] + 1) ** 2), c['ref']))
    if c['h'].virtual_decimation:
        seen(f'alpha left out, S = {c["s"]}', worst(wrong(c, alpha=[1.0] * c['C']), c['ref']))


def test_tolerance_sees_sigma_for_sigma_squared_ssd():
    c = host_case(SSD)
    h = R.Hyper(**{**c['h'].__dict__, 'ssd_inv_sigma': c['h'].ssd_inv_sigma ** 0.5})
    seen('SSD: sigma for sigma^2', worst(wrong(c, h=h), c['ref']))
    seen('SSD: alpha left out', worst(wrong(c, alpha=[1.0] * c['C']), c['ref']))
