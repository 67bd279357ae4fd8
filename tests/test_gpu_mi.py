"""The MI data term on the GPU (csrc/mi_kernels.hip) against the float64 restatement of tests/_mi.py: the uint64 histogram EXACTLY, the
table, MI, the data term, the gradient and the pmi map element by element at the tolerances derived there; special inputs; the fused
transition against the composition of the stateless operators; refusals; the trainer; behaviour on the inverted-contrast pair.

Launch geometry (mi_blocks): min(ceil(units / 256), IRS_MI_MAX_BLOCKS / C) blocks per chain, units of four voxels when V % 4 == 0.
  (5,7,9)     315 voxels: the scalar form, two blocks, the last with 59 voxels;
  (4,6,8)     192 voxels: the vector form, 48 units in one block;
  (9,11,13)   1287 voxels: six blocks, the last ragged (7 voxels);
  (33,33,33)  35 937 voxels, 8 chains: scalar, past the cap of 1024 / 8 = 128 blocks x 256 voxels = 32 768 -- a second, ragged trip;
  (52,51,52)  137 904 voxels, 8 chains: vector, past 128 x 256 x 4 = 131 072."""
import copy
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from ir_sgmcmc_amd import _lib as L
from ir_sgmcmc_amd import mi, ops
from ir_sgmcmc_amd.engine import EngineConfig, TransitionEngine, irs_config
from tests import _data_gradient as G
from tests import _mi as M

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = np.float64
UNIT = (0.0, 1.0)


def name(dims, *rest):
    return '-'.join(['x'.join(map(str, dims))] + [str(r) for r in rest])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def hist_u64(t):
    return t.cpu().numpy().view(np.uint64)


def within(test, key, got, ref, tol):
    """|got - ref| <= tol at EVERY element; prints the largest share of the tolerance in use"""
    got, ref, tol = (np.asarray(x, F64) for x in (got, ref, tol))
    dev_ = np.abs(got - ref)
    zero = tol == 0
    assert not dev_[zero].any(), f'{test}: {key}: {int((dev_[zero] != 0).sum())} elements differ where the tolerance is 0'
    used = float((dev_[~zero] / tol[~zero]).max()) if (~zero).any() else 0.0
    print(f'{test}: {key}: {used:.4f} of the tolerance')
    assert used <= 1.0, f'{test}: {key}: {used} x the tolerance'
    return used


def make_mask(kind, shape, C, seed):
    if kind is None:
        return None
    rng = np.random.default_rng(seed)
    return rng.random((C if kind == 'per_chain' else 1, 1, *shape)) < 0.7


def hold_ops(test, fixed, moving, mask, bins, f_range, m_range, scale=None):
    """both operators against the restatement, chain by chain -> (the device's outputs, the restatement)"""
    C = moving.shape[0]
    fd, md, kd = dev(fixed), dev(moving), None if mask is None else dev(mask)
    out = mi.mi_forward(fd, md, kd, bins, f_range, m_range, want_hist=True)
    sc = None if scale is None else torch.tensor(scale, dtype=torch.float32, device=DEV)
    g, pmi = mi.mi_backward(fd, md, out['table'], kd, bins, f_range, m_range, scale=sc, want_pmi=True)
    # two calls give the same bits
    again = mi.mi_forward(fd, md, kd, bins, f_range, m_range, want_hist=True)
    g2, pmi2 = mi.mi_backward(fd, md, again['table'], kd, bins, f_range, m_range, scale=sc, want_pmi=True)
    for a, b in ((out['hist'], again['hist']), (out['table'], again['table']), (out['stats'], again['stats']), (g, g2), (pmi, pmi2)):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    refs = M.reference(fixed, moving, mask, bins, f_range, m_range)
    hist, stats = hist_u64(out['hist']), out['stats'].cpu().numpy()
    for c, ref in enumerate(refs):
        w = 1.0 if scale is None else float(np.float32(scale[c]))
        assert (hist[c] == ref['hist']).all(), f'{test}: chain {c}: {int((hist[c] != ref["hist"]).sum())} cells of the histogram differ'
        assert int(hist[c].sum(dtype=np.uint64)) == ref['n'] << 30
        assert (hist[c].sum(axis=1, dtype=np.uint64) == ref['counts_a'].astype(np.uint64) << np.uint64(30)).all()
        assert (stats[c, 0], stats[c, 1], stats[c, 2]) == (ref['n'], ref['n_nonfinite'], ref['n_clipped'])
        tag = f'{test}/chain{c}'
        within(tag, 'T', out['table'][c].cpu().numpy(), ref['T'], ref['tol_T'])
        within(tag, 'MI', stats[c, 3], ref['mi'], ref['tol_mi'])
        within(tag, 'H_f', stats[c, 4], ref['h_fixed'], ref['tol_h_fixed'])
        within(tag, 'H_m', stats[c, 5], ref['h_moving'], ref['tol_h_moving'])
        within(tag, 'data term', stats[c, 6], ref['data_term'], ref['tol_term'])
        within(tag, 'g', g[c, 0].cpu().numpy(), w * ref['g'], abs(w) * ref['tol_g'])
        within(tag, 'pmi', pmi[c, 0].cpu().numpy(), ref['pmi'], ref['tol_pmi'])
        assert stats[c, 6] >= 0.0 and np.isfinite(stats[c]).all()
    # chain c of a batch is the single-chain call
    if C > 1:
        c = C - 1
        one = lambda a: a if a is None or a.shape[0] == 1 else a[c:c + 1].contiguous()
        o1 = mi.mi_forward(one(fd), md[c:c + 1].contiguous(), one(kd), bins, f_range, m_range, want_hist=True)
        g1, p1 = mi.mi_backward(one(fd), md[c:c + 1].contiguous(), o1['table'], one(kd), bins, f_range, m_range,
                                scale=None if sc is None else sc[c:c + 1].contiguous(), want_pmi=True)
        for a, b in ((out['hist'][c], o1['hist'][0]), (out['table'][c], o1['table'][0]), (out['stats'][c], o1['stats'][0]), (g[c], g1[0]),
                     (pmi[c], p1[0])):
            assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))
    return {'g': g, 'pmi': pmi, **out}, refs


OPS_CASES = [
    # dims, C, bins, fixed per chain, mask (None | 'shared' | 'per_chain')
    ((5, 7, 9), 2, 8, False, 'shared'), ((5, 7, 9), 2, 32, True, 'per_chain'), ((5, 7, 9), 2, 64, False, None),
    ((4, 6, 8), 2, 64, False, None), ((4, 6, 8), 1, 32, False, 'shared'), ((4, 6, 8), 2, 8, True, 'per_chain'),
    ((9, 11, 13), 2, 32, True, 'shared'), ((9, 11, 13), 1, 64, False, 'per_chain'),
    ((33, 33, 33), 8, 32, False, 'shared'), ((52, 51, 52), 8, 8, True, None),
]


@pytest.mark.parametrize('case', OPS_CASES, ids=[name(*c) for c in OPS_CASES])
def test_operators_against_the_restatement(case):
    dims, C, bins, per_chain_fixed, mask_kind = case
    fixed, moving = M.pair(dims, C, seed=sum(dims) + bins, Cf=C if per_chain_fixed else 1)
    moving[:, 0, -1, -1, -3:] = np.float32(1.25)                      # a few clipped voxels in the last (ragged) block
    mask = make_mask(mask_kind, dims, C, 7)
    scale = [1.0, -2.5, 0.75, 3.0, 1.0, 0.5, 2.0, 1.5][:C] if bins == 32 else None
    hold_ops('mi/ops/' + name(*case), fixed, moving, mask, bins, UNIT, UNIT, scale)


def test_cap_is_passed_by_the_capped_shapes():
    """the accumulate grid's cap as the header exports it: the two large cases take a second, ragged trip of the grid-stride loop"""
    header = open(os.path.join(ROOT, 'include', 'irsgmcmc.h')).read()
    cap = int(re.search(r'#define IRS_MI_MAX_BLOCKS (\d+)', header).group(1))
    assert cap == L.IRS_MI_MAX_BLOCKS == 1024
    for dims, C, unit in (((33, 33, 33), 8, 1), ((52, 51, 52), 8, 4)):
        V = int(np.prod(dims))
        assert (V % 4 == 0) == (unit == 4)
        trip = (cap // C) * 256 * unit
        assert trip < V < 1.5 * trip and (V // unit) % 256 != 0


def test_constant_images():
    """a constant moving image (every lane of a wavefront hits the same four cells) and constant slabs of whole wavefronts inside a
    varying image: the exact histogram is what holds the same-cell adds"""
    dims, bins = (8, 16, 16), 32
    fixed, moving = M.pair(dims, 2, seed=3)
    fixed[:, :, :3] = np.float32(0.25)
    moving[0] = np.float32(0.5)                      # chain 0: constant everywhere
    moving[1, 0, :3] = np.float32(0.125)             # chain 1: a constant slab of whole wavefronts, the rest varying
    got, refs = hold_ops('mi/constant', fixed, moving, None, bins, UNIT, UNIT)
    assert refs[0]['mi'] < 1e-12 and abs(refs[0]['data_term'] - refs[0]['n'] * math.log(bins)) < 1e-6   # a constant image: MI = 0
    assert not got['g'][0].any()                                                                      # ... and no gradient


def test_special_inputs():
    dims, bins = (5, 7, 9), 16
    fixed, moving = M.pair(dims, 1, seed=5)
    m_range = (0.25, 0.75)
    flat = moving.reshape(-1)
    flat[0], flat[1] = np.float32(0.25), np.float32(0.75)             # exactly m_lo and m_hi: inside, u = 0 and the last interval's u = 1
    flat[2], flat[3] = np.float32(-3.0), np.float32(1e30)             # far outside: clipped, g = 0
    flat[4], flat[5] = np.float32('nan'), np.float32('inf')           # non-finite under the mask: excluded and counted
    fixed.reshape(-1)[6] = np.float32('nan')
    got, refs = hold_ops('mi/special', fixed, moving, None, bins, UNIT, m_range)
    ref = refs[0]
    assert ref['n_nonfinite'] == 3 and ref['n_clipped'] >= 2 and ref['inside'].reshape(-1)[[0, 1]].all()
    g = got['g'].cpu().numpy().reshape(-1)
    assert not g[2:7].any() and np.isfinite(g).all() and abs(g[0]) > 0
    # an empty mask: n = 0, data term 0, gradient 0, no NaN
    got, refs = hold_ops('mi/empty', fixed, moving, np.zeros((1, 1, *dims), bool), bins, UNIT, m_range)
    assert refs[0]['n'] == 0 and float(got['stats'][0, 6]) == 0.0 and not got['g'].any() and not got['table'].any()
    assert bool(torch.isfinite(got['stats']).all())
    # a single taking lane per wavefront
    mask = np.zeros(int(np.prod(dims)), bool)
    mask[7::64] = True
    got, refs = hold_ops('mi/one_lane', fixed, moving, mask.reshape(1, 1, *dims), bins, UNIT, m_range)
    assert refs[0]['n'] == int(mask.sum()) - int((~np.isfinite(moving.reshape(-1)[mask]) | ~np.isfinite(fixed.reshape(-1)[mask])).sum())


@pytest.mark.parametrize('bins', [8, 32])
def test_each_mistake_exceeds_the_tolerance_on_the_device_outputs(bins):
    """the device's g passes (above); the three seeded mistakes of the restatement would not, by a wide factor"""
    dims = (5, 7, 9)
    fixed, moving = M.pair(dims, 1, seed=9)
    m_range = (0.1, 0.9)
    got, refs = hold_ops(f'mi/mistakes{bins}', fixed, moving, None, bins, UNIT, m_range)
    g = got['g'][0, 0].cpu().numpy().astype(F64)
    for mistake in M.MISTAKES:
        wrong = M.reference_one(fixed[0, 0], moving[0, 0], None, bins, UNIT, m_range, mistake=mistake)
        some = refs[0]['tol_g'] > 0
        factor = float((np.abs(wrong['g'] - g)[some] / refs[0]['tol_g'][some]).max())
        print(f'mi/mistakes: {mistake}, {bins} bins: {factor:.3g} x the tolerance')
        assert factor > 1000.0


def test_default_ranges_and_wrapper_refusals():
    dims = (4, 6, 8)
    fixed, moving = M.pair(dims, 2, seed=11)
    mask = make_mask('shared', dims, 2, 3)
    fixed[0, 0, 0, 0, 0], moving[1, 0, 0, 0, 1] = np.float32('nan'), np.float32('inf')
    fd, md, kd = dev(fixed), dev(moving), dev(mask)
    out = mi.mi_forward(fd, md, kd, 16)
    fin = np.isfinite(fixed) & mask
    assert out['ranges'] == [float(fixed[fin].min()), float(fixed[fin].max()), float(moving[np.isfinite(moving)].min()),
                             float(moving[np.isfinite(moving)].max())]
    term, g = mi.mi_loss(fd, md, kd, 16)
    assert torch.equal(term, out['stats'][:, 6]) and g.shape == md.shape
    for bad in (7, 65, 8.0, True):
        with pytest.raises(L.IrsError, match='bins'):
            mi.mi_forward(fd, md, kd, bad)
    with pytest.raises(L.IrsError, match='hi > lo'):
        mi.mi_forward(fd, md, kd, 16, (0.0, 0.0), UNIT)
    with pytest.raises(L.IrsError, match='hi > lo'):
        mi.mi_forward(fd, md, kd, 16, UNIT, (0.0, float('inf')))
    with pytest.raises(L.IrsError, match='does not match'):
        mi.mi_forward(fd, md, torch.ones(3, 1, *dims, dtype=torch.bool, device=DEV), 16)
    with pytest.raises(L.IrsError, match='table'):
        mi.mi_backward(fd, md, torch.zeros(2, 8, 8, device=DEV), kd, 16, UNIT, UNIT)
    with pytest.raises(L.IrsError, match='GPU only'):
        mi.mi_forward(fd.cpu(), md.cpu(), None, 16, UNIT, UNIT)
    lib = L.load()
    scratch = torch.empty(L.IRS_MI_WS_BYTES, dtype=torch.uint8, device=DEV)
    table, stats = torch.empty(2, 16, 16, device=DEV), torch.empty(2, 7, dtype=torch.float64, device=DEV)
    args = lambda bins, lo, hi: (L.dev_ptr(fd), 1, L.dev_ptr(md), None, 1, bins, lo, hi, 0.0, 1.0, None, L.dev_ptr(table), L.dev_ptr(stats),
                                 L.dev_ptr(scratch), 2, *dims, L.stream_ptr())
    assert lib.irs_mi_fwd(*args(7, 0.0, 1.0)) != 0 and 'bins = 7, 8..64' in lib.irs_last_error().decode()
    assert lib.irs_mi_fwd(*args(16, 1.0, 1.0)) != 0 and 'fixed range' in lib.irs_last_error().decode()
    assert lib.irs_mi_fwd(*args(16, 0.0, float('nan'))) != 0 and 'fixed range' in lib.irs_last_error().decode()


def test_autograd_of_the_loss_class():
    from ir_sgmcmc_amd.model.loss import MI, DataLoss
    dims, C, bins, w = (5, 7, 9), 2, 16, 3.0
    loss = MI(bins=bins, weight=w, fixed_range=UNIT, moving_range=UNIT)
    assert isinstance(loss, DataLoss) and loss.no_components == 1
    fixed, moving = M.pair(dims, C, seed=13)
    mask = make_mask('shared', dims, C, 5)
    m = dev(moving).requires_grad_(True)
    total = loss(dev(fixed).expand(C, -1, -1, -1, -1), m, dev(mask).expand(C, -1, -1, -1, -1))
    (2.0 * total).backward()
    refs = M.reference(fixed, moving, mask, bins, UNIT, UNIT)
    within('mi/autograd', 'loss', float(total), w * sum(r['data_term'] for r in refs), w * sum(r['tol_term'] for r in refs))
    for c, r in enumerate(refs):
        within('mi/autograd', f'dL/dM chain {c}', m.grad[c, 0].cpu().numpy(), 2.0 * w * r['g'], 2.0 * w * r['tol_g'])


# ------------------------------------------------------------------------------------------------------------------------------
# the fused transition against the composition of the stateless operators
# ------------------------------------------------------------------------------------------------------------------------------
WEIGHT, BINS = 3.0, 16
# dims, C, cps.  At every shape grad_v is held per element against the composition of the stateless operators: mi_backward on the warped
# image the transition returns, warp_displacement_bwd, svf_exp_bwd and, for SVFFD, ffd_adjoint.  On a 2^k + 1 grid the warp at
# velocity zero returns the moving image itself and its adjoint reads the one-sided differences of tests/_data_gradient.py: there
# grad_v is held against that closed form as well.  (16^3 and 24^3 are no such grids -- a sample point may fall a rounding below its
# voxel -- and have V % 4 == 0: the vector form of the gradient kernel writes g_warped inside the transition.)
ENGINE_CASES = [((16, 16, 16), 1, None), ((16, 16, 16), 2, None), ((24, 24, 24), 1, None), ((24, 24, 24), 2, None),
                ((16, 16, 16), 2, (2, 2, 2)), ((24, 24, 24), 1, (3, 3, 3)), ((17, 17, 17), 2, None), ((9, 17, 33), 1, None),
                ((17, 17, 17), 1, (2, 2, 2)), ((17, 17, 17), 2, (2, 2, 2))]


def engine_inputs(dims, C, band=False):
    fixed, _ = G.smooth_fixed(dims, C)                 # a fixed image per chain
    mask = torch.ones(1, 1, *dims, dtype=torch.bool)
    if band:   # a few planes around D / 2: g_warped vanishes off them, the sparse adjoint's support
        mask[:, :, :dims[0] // 2 - 2] = False
        mask[:, :, dims[0] // 2 + 2:] = False
    else:
        mask[:, :, :, :2] = False
    return fixed.contiguous(), G.tri_image(dims), mask.contiguous()


def run_engine(dims, C, cps, band=False, sparse_adjoint=None):
    fixed, moving, mask = engine_inputs(dims, C, band)
    f_range = (float(fixed.min()), float(fixed.max()))
    m_range = (-1.0, 15.0)
    eng = TransitionEngine(EngineConfig(dims=dims, no_chains=C, cps=cps, sobolev_s=0, uniform_noise=0.0, lr=0.05, data_loss='MI',
                                        virtual_decimation=False, mi_bins=BINS, mi_weight=WEIGHT, mi_fixed_range=f_range,
                                        mi_moving_range=m_range), DEV)
    try:
        eng.option('predict_variants', 0)
        if sparse_adjoint is not None:
            eng.set_sparse_adjoint(sparse_adjoint)
        fd, md = eng.prepare({'im': fixed.to(DEV), 'mask': mask.to(DEV)}, {'im': moving.to(DEV)})
        nan = lambda *shape: torch.full(shape, float('nan'), device=DEV, dtype=torch.float32)
        dv = eng.cfg.dims_v
        out = {'residuals': nan(C, 1, *dims), 'grad_v': nan(C, 3, *dv), 'im_moving_warped': nan(C, 1, *dims), 'displacement': nan(C, 3, *dims)}
        v = torch.zeros(C, 3, *dv, device=DEV)
        eng.transition(fd, md, v, None, torch.zeros(C, 3, *dv, device=DEV), None, out)
        sc = eng.scalars()
        res = {k: t.clone() for k, t in out.items()}
        res.update(scalars=sc, v_new=v.clone(), engaged=max(e['engaged'] for step in eng.sparse_adjoint() for e in step),
                   ranges=(f_range, m_range), inputs=(fixed, moving, mask))
        with pytest.raises(L.IrsError, match='only before the first transition'):
            eng.mi_set(WEIGHT, f_range, m_range)
        return res
    finally:
        eng.__del__()


@pytest.mark.parametrize('case', ENGINE_CASES, ids=[name(*c) for c in ENGINE_CASES])
def test_transition_equals_the_operators(case):
    dims, C, cps = case
    res = run_engine(dims, C, cps)
    fixed, moving, mask = res['inputs']
    f_range, m_range = res['ranges']
    T = 'mi/transition/' + name(*case)
    warped = res['im_moving_warped']
    exact_grid = all(n - 1 == 1 << int(math.log2(n - 1)) for n in dims)
    assert int(torch.count_nonzero(res['displacement'])) == 0   # v = 0
    assert not exact_grid or torch.equal(warped.cpu(), moving.expand(C, -1, -1, -1, -1))
    fd, kd = fixed.to(DEV), mask.to(DEV)
    out = mi.mi_forward(fd, warped, kd, BINS, f_range, m_range)
    g, pmi = mi.mi_backward(fd, warped, out['table'], kd, BINS, f_range, m_range, want_pmi=True)
    # g_warped of the transition: the same kernel with the weight as the chain's scale -- the same coefficient, the same bits
    g_warped = mi.mi_backward(fd, warped, out['table'], kd, BINS, f_range, m_range, scale=torch.full((C,), WEIGHT, device=DEV))
    # the data term of the transition IS weight * (the operator's term on the warped image it returns): the same kernels, the same bits
    assert res['scalars']['data_term'] == [WEIGHT * float(x) for x in out['stats'][:, 6]]
    assert res['scalars']['alpha'] == [1.0] * C and res['scalars']['n_mask'] == [float(mask.sum())] * C
    # residuals = mask (ln B - pmi): one float32 rounding of a float64 difference against the float32 difference formed here
    take = (kd != 0).expand(C, -1, -1, -1, -1)
    ref_res = torch.where(take, math.log(BINS) - pmi.double(), torch.zeros((), dtype=torch.float64, device=DEV))
    within(T, 'residuals', res['residuals'].cpu().numpy(), ref_res.cpu().numpy(), (2.0 ** -23 * (math.log(BINS) + pmi.abs().double())).cpu().numpy())
    total = WEIGHT * res['residuals'].double().sum(dim=(1, 2, 3, 4))
    # (every residual rounded to float32 once; and pmi uses the weights w_j where the term has their fixed point q_j / 2^30, at most
    # 2^-31 away, three times that for q_1: six of them per voxel at most max|T| each)
    n_take = take.double().sum(dim=(1, 2, 3, 4))
    t_max = out['table'].abs().double().amax(dim=(1, 2))
    tol_sum = WEIGHT * ((2.0 ** -24 * (math.log(BINS) + pmi.abs().double()) * take).sum(dim=(1, 2, 3, 4)) + n_take * 6 * 2.0 ** -31 * t_max)
    within(T, 'weight x masked sum of the residuals', total.cpu().numpy(), res['scalars']['data_term'], tol_sum.cpu().numpy())
    # grad_v at velocity zero: g_warped Delta_ch m (tests/_data_gradient.py), g_warped = weight * the operator's gradient
    gw = WEIGHT * g.double().cpu()
    dm = G.one_sided_differences(moving[0, 0].double()).unsqueeze(0)
    assert float(gw.abs().max()) > 1e-3
    expected = gw * dm
    # g_warped itself is the operator's, bit for bit (the same kernel); four float32 roundings on the way to grad_v (the product with
    # Delta m, the two prescale factors, the step) and the 8-tap cancellation of the warp adjoint, 8 U max|m| / |Delta m| relative
    tol = 4.0 * G.U * expected.abs() + 8.0 * G.U * float(moving.abs().max()) * gw.abs() * (dm != 0).double()
    grad = res['grad_v'].cpu()
    assert bool(torch.isfinite(grad).all())
    assert float(grad.abs().max()) > 0.0
    # the composition of the stateless operators, at any grid: g_warped -> warp adjoint -> adjoint of the 12 squaring steps (-> B-spline
    # adjoint).  The transition runs fused forms of the same steps (the warp adjoint folded into the first squaring step, interleaved
    # fields, the prescale inside the update): other roundings, not other numbers.  Bound: at velocity zero every one of these adjoints
    # has non-negative weights, so an error e >= 0 in dL/d(d_last) reaches grad_v as at most adjoint(e).  e: K U |g_d| for the
    # roundings of either path (12 steps x 16 for an 8-tap sum and its products, + 8 for the warp adjoint and the prescale: K = 200)
    # and the 8-tap cancellation of the warp adjoint, 8 U max|m| |g_warped| per voxel, (n - 1) / 2 times that in normalised units.
    zero = torch.zeros(C, 3, *dims, device=DEV)
    _, _, steps = ops.svf_exp_fwd(zero, 12, want_outputs=False)
    assert int(torch.count_nonzero(steps)) == 0
    d_last = steps[-1].contiguous()
    md = moving.to(DEV)
    g_d = ops.warp_displacement_bwd(md, d_last, g_warped)
    half = torch.tensor([(dims[2] - 1) / 2.0, (dims[1] - 1) / 2.0, (dims[0] - 1) / 2.0], device=DEV).view(1, 3, 1, 1, 1)   # x, y, z
    err_d = 200.0 * G.U * g_d.abs() + 8.0 * G.U * float(moving.abs().max()) * g_warped.abs() * half
    comp, comp_tol = ops.svf_exp_bwd(zero, steps, g_d), ops.svf_exp_bwd(zero, steps, err_d.contiguous())
    if cps is not None:
        n_terms = 3 * (4 * max(cps) - 1) + 4
        comp_tol = ops.ffd_adjoint((comp_tol + n_terms * G.U * comp.abs()).contiguous(), cps)
        comp = ops.ffd_adjoint(comp, cps)
    assert float(comp.abs().max()) > 1e-3
    print(f'{T}: grad_v against the composed operators: max |difference| {float((grad - comp.cpu()).abs().max()):.3g} at max |grad_v| '
          f'{float(grad.abs().max()):.3g}')
    within(T, 'grad_v against the composed operators', grad.numpy(), comp.cpu().numpy(), comp_tol.double().cpu().numpy() * (1 + 1e-6) + 1e-30)
    if not exact_grid:
        pass
    elif cps is None:
        for ch in range(3):
            within(T, f'grad_v channel {ch}', grad[:, ch].numpy(), expected[:, ch].numpy(), tol[:, ch].numpy())
    else:   # SVFFD: the B-spline adjoint of the same dense gradient; its taps are >= 0: the bound goes through it
        exp_cp = ops.ffd_adjoint(expected.float().to(DEV).contiguous(), cps).cpu().double()
        n_terms = 3 * (4 * max(cps) - 1) + 4
        tol_cp = ops.ffd_adjoint((tol + n_terms * G.U * expected.abs()).float().to(DEV).contiguous(), cps).cpu().double() * (1 + 1e-6)
        within(T, 'grad_v on the control grid', grad.numpy(), exp_cp.numpy(), tol_cp.numpy() + 1e-30)
    assert torch.equal(res['v_new'].cpu(), -(torch.tensor(0.05, dtype=torch.float32) * grad))


@pytest.fixture
def short_adjoint_pieces():
    L.option_set('march_seg', 8)     # process-wide: the adjoint's piece length, so that lists exist on volumes this small
    yield
    L.option_set('march_seg', 0)


@pytest.mark.parametrize('case', [((33, 5, 65), 1, None), ((17, 33, 65), 2, None)], ids=lambda c: name(*c))
def test_sparse_adjoint_does_not_change_a_bit(case, short_adjoint_pieces):
    dims, C, cps = case
    on, off = run_engine(dims, C, cps, band=True), run_engine(dims, C, cps, band=True, sparse_adjoint=False)
    assert on['engaged'] == 1 and off['engaged'] == 0
    for k in ('grad_v', 'residuals', 'v_new', 'im_moving_warped'):
        assert torch.equal(on[k], off[k]), k
    assert on['scalars'] == off['scalars'] and float(on['grad_v'].abs().max()) > 0.0


def refused(lib, cfg):
    import ctypes as C
    ctx = C.c_void_p()
    assert lib.irs_create(C.byref(cfg), C.byref(ctx)) != 0 and not ctx.value
    return lib.irs_last_error().decode()


def test_refusals():
    import ctypes as C
    lib = L.load()
    base = dict(dims=(16, 16, 16), data_loss='MI', mi_bins=16, virtual_decimation=False)
    assert 'virtual decimation' in refused(lib, irs_config(EngineConfig(**{**base, 'virtual_decimation': True})))
    for b in (7, 65):
        assert 'MI bins' in refused(lib, irs_config(EngineConfig(**{**base, 'mi_bins': b})))
    cfg = irs_config(EngineConfig(**base))
    cfg.data_loss = 2       # reserved
    assert refused(lib, cfg) == 'irs_create: unknown data loss'
    cfg, ctx, scfg = irs_config(EngineConfig(**base)), C.c_void_p(), L.IrsSlabConfig(0, 0)
    assert lib.irs_slab_create(C.byref(cfg), C.byref(scfg), None, C.byref(ctx)) != 0 and not ctx.value
    msg = lib.irs_last_error().decode()
    from ir_sgmcmc_amd.slab import SlabEngine
    with pytest.raises(L.IrsError) as err:
        SlabEngine(EngineConfig(**base), DEV)
    assert str(err.value) == msg and 'MI data term' in msg
    # a context that never had irs_mi_set: its first transition is refused, with the reason
    eng = TransitionEngine(EngineConfig(**base), DEV)
    fixed, moving, mask = engine_inputs((16, 16, 16), 1)
    fd, md = eng.prepare({'im': fixed.to(DEV), 'mask': mask.to(DEV)}, {'im': moving.to(DEV)})
    with pytest.raises(L.IrsError, match='needs irs_mi_set'):
        eng.transition(fd, md, torch.zeros(1, 3, 16, 16, 16, device=DEV))
    for w, fr, mr in ((0.0, UNIT, UNIT), (float('nan'), UNIT, UNIT), (1.0, (1.0, 1.0), UNIT), (1.0, UNIT, (2.0, 1.0)),
                      (1.0, (0.0, float('inf')), UNIT), (1.0, UNIT, (float('nan'), 1.0))):
        with pytest.raises(L.IrsError, match='finite'):
            eng.mi_set(w, fr, mr)
    eng.mi_set(2.0, UNIT, (-1.0, 15.0))
    eng.transition(fd, md, torch.zeros(1, 3, 16, 16, 16, device=DEV))
    eng.flush()
    with pytest.raises(L.IrsError, match='only before the first transition'):
        eng.mi_set(2.0, UNIT, UNIT)
    other = TransitionEngine(EngineConfig(dims=(16, 16, 16), data_loss='SSD', virtual_decimation=False), DEV)
    with pytest.raises(L.IrsError, match='not IRS_DATA_MI'):
        other.mi_set(1.0, UNIT, UNIT)


# ------------------------------------------------------------------------------------------------------------------------------
# the trainer: the new config cut to 24^3 and ten transitions; checkpoint and resume
# ------------------------------------------------------------------------------------------------------------------------------
def make_trainer(tmp_path, top=None, **trainer_over):
    from ir_sgmcmc_amd.parse_config import ConfigParser
    from ir_sgmcmc_amd.trainer import Trainer
    cfg = json.load(open(os.path.join(ROOT, 'configs', 'synthetic_mi_l2_128.json')))
    cfg['trainer']['save_dir'] = str(tmp_path)
    cfg['data_loader']['args']['dims'] = [24, 24, 24]
    cfg['trainer'].update(no_iters_burn_in=4, no_samples_MCMC=6, log_period_MCMC=2, checkpoint_period=4)
    cfg['trainer'].update(trainer_over)
    cfg.update(top or {})
    config = ConfigParser.from_dict(copy.deepcopy(cfg), timestamp='t')
    dl = config.init_data_loader()
    tm, rm = config.init_transformation_and_registration_modules()
    return Trainer(config, dl, config.init_losses(), tm, rm, config.init_metrics(), device=DEV)


def digest(t):
    s = t.engine.state()
    return (t.v_curr_state.cpu(), t.displacement_mean.cpu(), t.displacement_std.cpu(), s.iteration, list(s.reg_param))


def test_trainer_runs_the_config_and_resumes_bit_for_bit(tmp_path):
    a = make_trainer(tmp_path / 'a')
    torch.manual_seed(0)
    a.run()
    a.engine.flush()
    ec = a.engine.cfg
    cfg = json.load(open(os.path.join(ROOT, 'configs', 'synthetic_mi_l2_128.json')))['data_loss']['args']
    assert (ec.data_loss, ec.mi_bins, ec.mi_weight) == ('MI', cfg['bins'], cfg['weight'])
    f_range, m_range = mi.mi_ranges(a._fixed['im'], a._moving['im'], a._fixed['mask'])
    assert (tuple(ec.mi_fixed_range), tuple(ec.mi_moving_range)) == (f_range, m_range)      # computed once, from the pair of the chains
    assert bool(torch.isfinite(a.v_curr_state).all()) and float(a.v_curr_state.abs().max()) > 0.0
    term, _ = mi.mi_loss(a._fixed['im'], a._outputs['im_moving_warped'], a._fixed['mask'], ec.mi_bins, f_range, m_range)
    weight = float(np.float32(ec.mi_weight))        # (irs_mi_set takes the weight as a float)
    assert a.engine.scalars()['data_term'] == [weight * float(x) for x in term]
    ck = a.config.save_dirs['checkpoints'] / 'checkpoint_0000004.pt'
    assert ck.is_file()
    b = make_trainer(tmp_path / 'b', resume=str(ck))
    torch.manual_seed(0)
    b.run()
    assert all(torch.equal(x, z) if isinstance(x, torch.Tensor) else x == z for x, z in zip(digest(a), digest(b)))


def test_trainer_refusals(tmp_path):
    with pytest.raises(ValueError, match='virtual decimation'):
        make_trainer(tmp_path / 'a', top={'virtual_decimation': True})._engine_config()
    with pytest.raises(ValueError, match='residual_check'):
        make_trainer(tmp_path / 'b', residual_check={'bins': 32})._engine_config()
    with pytest.raises(ValueError, match='VI stage'):
        make_trainer(tmp_path / 'c', VI=True)._engine_config()


# ------------------------------------------------------------------------------------------------------------------------------
# behaviour on the inverted-contrast pair
# ------------------------------------------------------------------------------------------------------------------------------
BEHAVIOUR = dict(dims=(32, 32, 32), weight=1.0, lr=0.4, transitions=40, seed=0)


def test_chain_registers_the_inverted_pair():
    """32^3, synthetic_pair(seed 0, moving_contrast "invert"), 32 bins, weight, step size and transition count of BEHAVIOUR: the chain's
    data term falls below its first value, and the MI of ops.image_similarity -- an independent estimator with hard bins -- between the
    fixed and the warped moving image rises above that of the unregistered pair.  Measured on the MI355X: data term 34 730 -> 28 487,
    hard-bin MI 0.903 -> 1.439.  An SSD chain (sigma 0.1) with the same step size and count on the same pair lowers its own data term
    (511 858 -> 25 084) while that MI FALLS from 0.903 to 0.308: it pulls the wrong way (not asserted)."""
    from ir_sgmcmc_amd.data_loader import synthetic_pair
    dims = BEHAVIOUR['dims']
    f1, m1 = synthetic_pair(dims, seed=BEHAVIOUR['seed'], moving_contrast='invert')
    fixed = {k: v.unsqueeze(0).to(DEV) for k, v in f1.items() if k != 'seg'}
    moving = {k: v.unsqueeze(0).to(DEV) for k, v in m1.items() if k != 'seg'}
    f_range, m_range = mi.mi_ranges(fixed['im'], moving['im'], fixed['mask'])
    eng = TransitionEngine(EngineConfig(dims=dims, lr=BEHAVIOUR['lr'], seed=BEHAVIOUR['seed'], data_loss='MI', virtual_decimation=False,
                                        mi_bins=32, mi_weight=BEHAVIOUR['weight'], mi_fixed_range=f_range, mi_moving_range=m_range), DEV)
    fd, md = eng.prepare(fixed, moving)
    v = torch.zeros(1, 3, *dims, device=DEV)
    warped = torch.empty(1, 1, *dims, device=DEV)
    terms = []
    for it in range(BEHAVIOUR['transitions']):
        eng.transition(fd, md, v, None, None, None, {'im_moving_warped': warped})
        if it in (0, BEHAVIOUR['transitions'] - 1):
            eng.flush()
            terms.append(eng.scalars()['data_term'][0])
    col = ops.SIMILARITY_COLUMNS.index('mi')
    before = float(ops.image_similarity(fixed['im'], moving['im'], fixed['mask'], 32)['stats'][0, col])
    after = float(ops.image_similarity(fixed['im'], warped, fixed['mask'], 32)['stats'][0, col])
    print(f'mi/behaviour: data term {terms[0]:.6g} -> {terms[1]:.6g}; hard-bin MI {before:.6g} -> {after:.6g}')
    assert terms[1] < terms[0] and after > before
