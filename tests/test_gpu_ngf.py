"""The NGF data term on the GPU (csrc/ngf_kernels.hip, csrc/ngf_device.h) against the float32 restatement of tests/_ngf.py, BIT FOR
BIT: the two operators, the special inputs, the data stage of a transition against the stateless operators, the sparse adjoint, the
default path left alone, recovery and stream capture, the autograd layer, the refusals, the trainer and one behaviour run.

Geometry of the two kernels: a workgroup owns a 32 x 8 column tile with a halo of one voxel and marches a z segment with a run-in of
one plane; by size a segment is at least 4 planes long (`lcc_seg` forces a length).  The shapes (D,H,W) in those terms:
  (2,2,2)     the smallest legal volume: both face rules of grad^T and nothing else, on all three axes;
  (3,3,3)     one interior voxel per axis between the two faces;
  (2,5,6)     n = 2 along the marched axis only;
  (5,9,33)    crosses a tile edge in y and in x by one voxel: a second tile row of one row, a second tile column of one column;
  (7,17,70)   three x tiles and three y tiles, the last ragged; segments 4 + 3;
  (7,17,70) with lcc_seg = 2 and 3: seams on odd and on even planes, a last segment of one plane."""
import contextlib
import copy
import ctypes as C
import gc
import json
import math
import os

import numpy as np
import pytest
import torch

from ir_sgmcmc_amd import _lib as L
from ir_sgmcmc_amd import ngf, ops
from ir_sgmcmc_amd.engine import EngineConfig, TransitionEngine, irs_config
from tests import _data_gradient as G
from tests import _ngf as N

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = (0.3, 0.41)


def name(dims, *rest):
    return '-'.join(['x'.join(map(str, dims))] + [str(r) for r in rest])


def within(test, key, got, ref, tol):
    """|got - ref| <= tol at EVERY element; prints the largest share of the tolerance in use"""
    got, ref, tol = (np.asarray(x.detach().cpu() if torch.is_tensor(x) else x, np.float64) for x in (got, ref, tol))
    dev_ = np.abs(got - ref)
    zero = tol == 0
    assert not dev_[zero].any(), f'{test}: {key}: {int((dev_[zero] != 0).sum())} elements differ where the tolerance is 0'
    used = float((dev_[~zero] / tol[~zero]).max()) if (~zero).any() else 0.0
    print(f'{test}: {key}: {used:.4f} of the tolerance')
    assert used <= 1.0, f'{test}: {key}: {used} x the tolerance'
    return used


def same_bits(test, key, got, ref):
    got, ref = got.detach().cpu(), ref.detach().cpu()
    differ = int((got.view(torch.int32) != ref.view(torch.int32)).sum()) if got.dtype == torch.float32 else int((got != ref).sum())
    # (+0 and -0 are the same number but not the same bits: the restatement has to get the sign of a zero right too)
    print(f'{test}: {key}: {differ} of {got.numel()} elements differ in their bits')
    assert got.shape == ref.shape and differ == 0, f'{test}: {key}: {differ} elements differ'


@contextlib.contextmanager
def lcc_seg(n):
    """the process-wide segment length of the LCC / LNCC / NGF kernels; it may only change while no context is alive"""
    gc.collect()
    if n:
        L.option_set('lcc_seg', n)
    try:
        yield
    finally:
        gc.collect()
        if n:
            L.option_set('lcc_seg', 0)


# ------------------------------------------------------------------------------------------------------------------------------
# the two stateless operators
# ------------------------------------------------------------------------------------------------------------------------------
# the whole grid: dims x C x fixed per chain x upstream (None | 'shared' | 'per_chain'), lcc_seg 0; at (7,17,70) also lcc_seg 2 and 3
OPS_CASES = [(dims, Cn, per_chain, up, seg)
             for dims in ((2, 2, 2), (3, 3, 3), (2, 5, 6), (5, 9, 33), (7, 17, 70)) for Cn in (1, 3) for per_chain in (False, True)
             for up in (None, 'shared', 'per_chain') for seg in ((0, 2, 3) if dims == (7, 17, 70) else (0,))]


def ops_inputs(dims, Cn, per_chain_fixed, upstream):
    fixed, moving = N.images(dims, Cn)
    u = None if upstream is None else N.upstream(dims, Cn if upstream == 'per_chain' else 1)
    return (fixed if per_chain_fixed else fixed[:1]).contiguous(), moving, u


@pytest.mark.parametrize('dims,Cn,per_chain_fixed,upstream,seg', OPS_CASES, ids=[name(*c) for c in OPS_CASES])
def test_operators_bit_for_bit(dims, Cn, per_chain_fixed, upstream, seg):
    fixed, moving, u = ops_inputs(dims, Cn, per_chain_fixed, upstream)
    fd, md, ud = fixed.to(DEV), moving.to(DEV), None if u is None else u.to(DEV)
    with lcc_seg(seg):
        out = ngf.ngf_forward(fd, md, *EPS, ud)
        g = ngf.ngf_backward(out['coef'])
        again = ngf.ngf_forward(fd, md, *EPS, ud)
        g_again = ngf.ngf_backward(again['coef'])
        sums2, g2 = ngf.ngf_loss(fd, md, *EPS, ud)
        single = []
        for c in range(Cn):
            fc = fd[c:c + 1] if per_chain_fixed else fd
            uc = None if ud is None else (ud[c:c + 1] if ud.shape[0] > 1 else ud)
            oc = ngf.ngf_forward(fc, md[c:c + 1], *EPS, uc)
            single.append((oc, ngf.ngf_backward(oc['coef'])))
    ref = N.restate32(fixed, moving, u, *EPS)
    T = 'ngf/operators/' + name(dims, Cn, per_chain_fixed, upstream, seg)
    assert out['d'].dtype == torch.float32 and out['sums'].dtype == F64 and tuple(out['coef'].shape) == (Cn, 3, *dims)
    assert float(ref['g'].abs().max()) > 1e-3
    same_bits(T, 'd', out['d'], ref['d'])
    same_bits(T, 'c', out['coef'], ref['coef'])
    same_bits(T, 'g', g, ref['g'])
    # the sums: 1e-5 of sum |u| d, the project's loss tolerance, against a float64 sum of the restatement's d
    uu = torch.ones(1, 1, *dims) if u is None else u
    exact, scale = N.loss_sums(uu, ref['d']), N.loss_sums(uu.abs(), ref['d'].abs())
    within(T, 'sums', out['sums'], exact, N.LOSS_RTOL * scale)
    # no atomics, a fixed order of every sum: the same bits again, and chain c of the batch is the single-chain call
    for k in ('d', 'coef', 'sums'):
        assert torch.equal(out[k], again[k]), k
    assert torch.equal(g, g_again) and torch.equal(g, g2) and torch.equal(out['sums'], sums2)
    for c, (oc, gc_) in enumerate(single):
        for k in ('d', 'coef', 'sums'):
            assert torch.equal(out[k][c:c + 1], oc[k]), (k, c)
        assert torch.equal(g[c:c + 1], gc_), c


@pytest.mark.parametrize('dims', [(3, 9, 68), (4, 8, 64), (2, 17, 32)], ids=lambda d: name(d))
def test_adjoint_vector_staging_bit_for_bit(dims):
    """where W is a multiple of 4 the adjoint stages the c_y rows of its FULL tiles with 16-byte loads: (3,9,68) has two full x
    tiles and a ragged one of 4 columns, (4,8,64) and (2,17,32) full tiles only.  The same bits as the restatement, and as the
    4-byte path, which maps that do not start on a 16-byte boundary take."""
    fixed, moving, u = ops_inputs(dims, 2, True, 'per_chain')
    out = ngf.ngf_forward(fixed.to(DEV), moving.to(DEV), *EPS, u.to(DEV))
    ref = N.restate32(fixed, moving, u, *EPS)
    T = 'ngf/operators/vector-' + name(dims)
    same_bits(T, 'c', out['coef'], ref['coef'])
    same_bits(T, 'g', ngf.ngf_backward(out['coef']), ref['g'])
    flat = torch.empty(out['coef'].numel() + 1, device=DEV, dtype=torch.float32)
    shifted = flat[1:].view_as(out['coef'])      # the same maps one float off the allocation's alignment
    shifted.copy_(out['coef'])
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    same_bits(T, 'g from maps off the 16-byte boundary', ngf.ngf_backward(shifted), ref['g'])


def test_gpu_share_of_the_float64_bound():
    """bit-identical to the float32 restatement, the GPU uses the share of the derived float64 bound that the host test states for
    the restatement; measured here once more on the device's own output"""
    dims = (7, 17, 70)
    fixed, moving, u = ops_inputs(dims, 2, True, 'per_chain')
    out = ngf.ngf_forward(fixed.to(DEV), moving.to(DEV), *EPS, u.to(DEV))
    g = ngf.ngf_backward(out['coef'])
    ref = N.reference(fixed, moving, u, *EPS)
    T = 'ngf/operators/float64'
    within(T, 'd', out['d'], ref['d'], ref['tol']['d'])
    for i in range(3):
        within(T, f'c{i}', out['coef'][:, i:i + 1], ref['c'][i], ref['tol']['c'][i])
    within(T, 'g', g, ref['g'], ref['tol']['g'])


def test_optional_outputs_and_wrapper_checks():
    fixed, moving, u = ops_inputs((5, 9, 33), 2, False, 'per_chain')
    fd, md, ud = fixed.to(DEV), moving.to(DEV), u.to(DEV)
    out = ngf.ngf_forward(fd, md, *EPS, ud)
    only = ngf.ngf_forward(fd, md, *EPS, ud, want_map=False, want_coef=False)
    assert only['d'] is None and only['coef'] is None and torch.equal(only['sums'], out['sums'])
    no_sums = ngf.ngf_forward(fd, md, *EPS, ud, want_sums=False)
    assert no_sums['sums'] is None and torch.equal(no_sums['d'], out['d']) and torch.equal(no_sums['coef'], out['coef'])
    # the raw entry point with NULL outputs writes nothing: a canary behind each buffer it does get stays intact
    lib, V = L.load(), 5 * 9 * 33
    buf = torch.full((2 * V + 16,), 7.0, device=DEV)
    L.check(lib.irs_ngf_fwd(L.dev_ptr(fd), 1, L.dev_ptr(md), L.dev_ptr(ud), 2, EPS[0], EPS[1], L.dev_ptr(buf), None, None, None, 2, 5, 9, 33,
                            L.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(buf[:2 * V].view(2, 1, 5, 9, 33), out['d']) and bool((buf[2 * V:] == 7.0).all())
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(L.IrsError, match='finite value > 0'):
            ngf.ngf_forward(fd, md, bad, 0.1)
        with pytest.raises(L.IrsError, match='finite value > 0'):
            ngf.ngf_forward(fd, md, 0.1, bad)
    with pytest.raises(L.IrsError, match='does not match'):
        ngf.ngf_forward(fd, md, *EPS, upstream=torch.ones(3, 1, 5, 9, 33, device=DEV))
    with pytest.raises(L.IrsError, match='coef'):
        ngf.ngf_backward(torch.zeros(2, 2, 5, 9, 33, device=DEV))
    with pytest.raises(L.IrsError, match='float32'):
        ngf.ngf_forward(fd, md.double(), *EPS)


# ------------------------------------------------------------------------------------------------------------------------------
# special inputs
# ------------------------------------------------------------------------------------------------------------------------------
def test_constant_image_gives_one_and_zero():
    dims = (5, 9, 33)
    _, moving = N.images(dims, 2)
    flat = torch.full((1, 1, *dims), 0.75)
    for f, m in ((flat, moving), (moving[:1], flat.expand(2, -1, -1, -1, -1).contiguous()), (flat, flat)):
        out = ngf.ngf_forward(f.to(DEV), m.to(DEV), *EPS)
        g = ngf.ngf_backward(out['coef'])
        assert bool((out['d'] == 1.0).all()) and int(torch.count_nonzero(g)) == 0 and int(torch.count_nonzero(out['coef'])) == 0
        assert out['sums'].tolist() == [float(5 * 9 * 33)] * m.shape[0]


def test_identical_images():
    dims = (5, 9, 33)
    _, moving = N.images(dims, 1)
    out = ngf.ngf_forward(moving.to(DEV), moving.to(DEV), *EPS)
    g = ngf.ngf_backward(out['coef'])
    ref = N.restate32(moving, moving, None, *EPS)
    same_bits('ngf/identical', 'd', out['d'], ref['d'])
    same_bits('ngf/identical', 'g', g, ref['g'])
    assert bool(torch.isfinite(g).all()) and float(out['d'].max()) < 1.0 and float(out['d'].min()) >= 0.0


def test_a_nan_stays_within_the_stencil():
    """a NaN in M reaches d and c at its six axis neighbours (the central difference does not read the centre) and g at theirs"""
    dims, at = (7, 17, 70), (3, 8, 32)     # the voxel right of a tile seam in x (32) and below one in y (8), next to a z seam (4)
    fixed, moving, u = ops_inputs(dims, 1, False, 'per_chain')
    bad = moving.clone()
    bad[0, 0][at] = float('nan')
    clean = ngf.ngf_forward(fixed.to(DEV), moving.to(DEV), *EPS, u.to(DEV))
    out = ngf.ngf_forward(fixed.to(DEV), bad.to(DEV), *EPS, u.to(DEV))
    g_clean, g = ngf.ngf_backward(clean['coef']).cpu(), ngf.ngf_backward(out['coef']).cpu()
    zz, yy, xx = torch.meshgrid(*(torch.arange(n) for n in dims), indexing='ij')
    l1 = (zz - at[0]).abs() + (yy - at[1]).abs() + (xx - at[2]).abs()
    changed = lambda a, b: (a.view(torch.int32) != b.view(torch.int32))
    d_changed = changed(out['d'].cpu(), clean['d'].cpu())[0, 0]
    c_changed = changed(out['coef'].cpu(), clean['coef'].cpu())[0].any(0)
    g_changed = changed(g, g_clean)[0, 0]
    assert int(d_changed.sum()) == 6 and bool((l1[d_changed] == 1).all()) and bool(out['d'].cpu()[0, 0][d_changed].isnan().all())
    assert bool((l1[c_changed] == 1).all()) and int(c_changed.sum()) == 6
    assert int(g_changed.sum()) > 0 and bool((l1[g_changed] <= 2).all()) and bool(g[0, 0][g_changed].isnan().all())
    assert bool(torch.isfinite(g[0, 0][~g_changed]).all())


# ------------------------------------------------------------------------------------------------------------------------------
# the data stage of a transition against the stateless operators on the warped image it returns
# ------------------------------------------------------------------------------------------------------------------------------
WEIGHT = 4.0   # a power of two: weight * x is exact, so the transition's scalars and g_warped are the operators' bit for bit
ENGINE_CASES = [(dims, Cn, cps) for dims in ((16, 16, 16), (24, 24, 24)) for Cn in (1, 2) for cps in (None, (2, 2, 2))]


def engine_inputs(dims, Cn, band=False):
    fixed, _ = G.smooth_fixed(dims, Cn)                 # a fixed image per chain
    mask = torch.ones(1, 1, *dims, dtype=torch.bool)
    if band:   # a few planes around D / 2: g_warped vanishes two planes off them, the sparse adjoint's support
        mask[:, :, :dims[0] // 2 - 2] = False
        mask[:, :, dims[0] // 2 + 2:] = False
    else:
        mask[:, :, :, :2] = False
    return fixed.contiguous(), G.tri_image(dims), mask.contiguous()


def run_engine(dims, Cn, cps, band=False, sparse_adjoint=None):
    fixed, moving, mask = engine_inputs(dims, Cn, band)
    eps = ngf.ngf_edge_parameters(fixed, moving, mask)
    eng = TransitionEngine(EngineConfig(dims=dims, no_chains=Cn, cps=cps, sobolev_s=0, uniform_noise=0.0, lr=0.05, data_loss='NGF',
                                        virtual_decimation=False, ngf_weight=WEIGHT, ngf_fixed_eps=eps[0], ngf_moving_eps=eps[1]), DEV)
    try:
        eng.option('predict_variants', 0)   # every kernel variant is launched: nothing is assumed, no transition is re-run
        if sparse_adjoint is not None:
            eng.set_sparse_adjoint(sparse_adjoint)
        fd, md = eng.prepare({'im': fixed.to(DEV), 'mask': mask.to(DEV)}, {'im': moving.to(DEV)})
        nan = lambda *shape: torch.full(shape, float('nan'), device=DEV, dtype=torch.float32)
        dv = eng.cfg.dims_v
        out = {'residuals': nan(Cn, 1, *dims), 'grad_v': nan(Cn, 3, *dv), 'im_moving_warped': nan(Cn, 1, *dims), 'displacement': nan(Cn, 3, *dims)}
        v = torch.zeros(Cn, 3, *dv, device=DEV)
        eng.transition(fd, md, v, None, torch.zeros(Cn, 3, *dv, device=DEV), None, out)
        sc = eng.scalars()
        res = {k: t.clone() for k, t in out.items()}
        res.update(scalars=sc, v_new=v.clone(), engaged=max(e['engaged'] for step in eng.sparse_adjoint() for e in step), eps=eps,
                   inputs=(fixed, moving, mask))
        with pytest.raises(L.IrsError, match='only before the first transition'):
            eng.ngf_set(WEIGHT, *eps)
        return res
    finally:
        eng.__del__()


@pytest.mark.parametrize('case', ENGINE_CASES, ids=[name(*c) for c in ENGINE_CASES])
def test_transition_equals_the_operators(case):
    dims, Cn, cps = case
    res = run_engine(dims, Cn, cps)
    fixed, moving, mask = res['inputs']
    T = 'ngf/transition/' + name(*case)
    warped = res['im_moving_warped']
    assert int(torch.count_nonzero(res['displacement'])) == 0   # v = 0
    fd, u = fixed.to(DEV), mask.to(DEV).to(torch.float32)
    out = ngf.ngf_forward(fd, warped, *res['eps'], u)
    # the data term of the transition IS weight * (the operator's sum on the warped image it returns): the same kernel, the same
    # partials times a power of two, the same order of their sum
    assert res['scalars']['data_term'] == [WEIGHT * float(x) for x in out['sums']]
    assert res['scalars']['alpha'] == [1.0] * Cn and res['scalars']['n_mask'] == [float(mask.sum())] * Cn
    assert torch.equal(res['residuals'], u * out['d'])          # residuals = mask * d
    g_warped = (WEIGHT * ngf.ngf_backward(out['coef'])).contiguous()   # what the adjoint kernel writes with scale = weight, exactly
    assert float(g_warped.abs().max()) > 1e-3
    grad = res['grad_v'].cpu()
    assert bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0.0
    # the composition of the stateless operators: g_warped -> warp adjoint -> adjoint of the 12 squaring steps (-> B-spline adjoint).
    # The transition runs fused forms of the same steps (the warp adjoint folded into the first squaring step, interleaved fields,
    # the prescale inside the update): other roundings, not other numbers.  Bound (the argument of
    # test_gpu_mi.py::test_transition_equals_the_operators): at velocity zero every one of these adjoints has non-negative weights,
    # so an error e >= 0 in dL/d(d_last) reaches grad_v as at most adjoint(e).  e: K U |g_d| for the roundings of either path (12
    # steps x 16 for an 8-tap sum and its products, + 8 for the warp adjoint and the prescale: K = 200) and the 8-tap cancellation of
    # the warp adjoint, 8 U max|m| |g_warped| per voxel, (n - 1) / 2 times that in normalised units.
    zero = torch.zeros(Cn, 3, *dims, device=DEV)
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
    within(T, 'grad_v against the composed operators', grad, comp, comp_tol.double().cpu() * (1 + 1e-6) + 1e-30)
    assert torch.equal(res['v_new'].cpu(), -(torch.tensor(0.05, dtype=torch.float32) * grad))


@pytest.fixture
def short_adjoint_pieces():
    L.option_set('march_seg', 8)     # process-wide: the adjoint's piece length, so that lists exist on volumes this small
    yield
    L.option_set('march_seg', 0)


@pytest.mark.parametrize('case', [((33, 5, 65), 1, None), ((17, 33, 65), 2, None)], ids=lambda c: name(*c))
def test_sparse_adjoint_does_not_change_a_bit(case, short_adjoint_pieces):
    dims, Cn, cps = case
    on, off = run_engine(dims, Cn, cps, band=True), run_engine(dims, Cn, cps, band=True, sparse_adjoint=False)
    assert on['engaged'] == 1 and off['engaged'] == 0
    for k in ('grad_v', 'residuals', 'v_new', 'im_moving_warped'):
        assert torch.equal(on[k], off[k]), k
    assert on['scalars'] == off['scalars'] and float(on['grad_v'].abs().max()) > 0.0


# ------------------------------------------------------------------------------------------------------------------------------
# the default path, recovery, stream capture (tests/test_gpu_lncc.py)
# ------------------------------------------------------------------------------------------------------------------------------
def to_dev(d):
    return {k: v.to(DEV).contiguous() for k, v in d.items()}


def pair24():
    from ir_sgmcmc_amd.data_loader import synthetic_pair
    f1, m1 = synthetic_pair((24, 24, 24), seed=0)
    return (to_dev({k: v.unsqueeze(0) for k, v in f1.items() if k != 'seg'}), to_dev({k: v.unsqueeze(0) for k, v in m1.items() if k != 'seg'}))


def ngf24(seed, **kw):
    kw = {'ngf_weight': 10.0, 'ngf_fixed_eps': 0.02, 'ngf_moving_eps': 0.02, **kw}
    return TransitionEngine(EngineConfig(dims=(24, 24, 24), seed=seed, data_loss='NGF', virtual_decimation=False, **kw), DEV)


def chain(eng, fixed, moving, T=3):
    fd, md = eng.prepare(fixed, moving)
    if eng.cfg.data_loss == 'GMM':
        eng.gmm_init(fd, md)
    v = torch.zeros(eng.cfg.no_chains, 3, 24, 24, 24, device=DEV)
    for _ in range(T):
        eng.transition(fd, md, v)
    eng.flush()
    return v.clone(), eng.scalars()


def test_default_path_unchanged():
    fixed, moving = pair24()
    cfgs = [EngineConfig(dims=(24, 24, 24), seed=5), EngineConfig(dims=(24, 24, 24), seed=5, data_loss='SSD', virtual_decimation=False)]
    before = [chain(TransitionEngine(c, DEV), fixed, moving) for c in cfgs]
    v_n, _ = chain(ngf24(5), fixed, moving)
    assert bool(torch.isfinite(v_n).all()) and not torch.equal(v_n, before[1][0])
    after = [chain(TransitionEngine(c, DEV), fixed, moving) for c in cfgs]
    for (v0, s0), (v1, s1) in zip(before, after):
        assert torch.equal(v0, v1) and s0 == s1 and float(v0.abs().max()) > 0.0


def test_misprediction_is_recovered_on_an_ngf_chain():
    from ir_sgmcmc_amd.ops import perturb_smooth, sobolev_kernel_1d
    Nn, T = 24, 6
    fixed, moving = pair24()
    v0 = perturb_smooth(torch.randn(1, 3, Nn, Nn, Nn, generator=torch.Generator().manual_seed(3)).to(DEV), sobolev_kernel_1d(3, 0.5))
    v0 = v0 * (9.0 / float(v0.abs().max()))
    res = {}
    for mode in (0, 3):
        eng = ngf24(11)
        eng.option('predict_variants', mode)
        fd, md = eng.prepare(fixed, moving)
        v = v0.clone()
        for _ in range(T):
            eng.transition(fd, md, v)
        eng.flush()
        assert eng.state().iteration == T
        sc = eng.scalars()
        res[mode] = (v.clone(), sc['data_term'], sc['reg_energy'], eng.recovered_transitions)
    assert res[0][3] == 0 and res[3][3] >= 1, (res[0][3], res[3][3])
    assert torch.equal(res[0][0], res[3][0]) and res[0][1] == res[3][1] and res[0][2] == res[3][2]
    assert not torch.equal(res[0][0], v0) and math.isfinite(res[0][1][0])


def test_captured_transition_matches_an_eager_one():
    Nn = 24
    fixed, moving = pair24()

    def fresh():
        eng = ngf24(7)
        fd, md = eng.prepare(fixed, moving)
        return eng, fd, md

    eng, fd, md = fresh()
    v_plain = torch.zeros(1, 3, Nn, Nn, Nn, device=DEV)
    for _ in range(4):
        eng.transition(fd, md, v_plain)
    eng.flush()
    sc_plain = eng.scalars()

    eng, fd, md = fresh()
    v = torch.zeros(1, 3, Nn, Nn, Nn, device=DEV)
    eng.transition(fd, md, v)  # (lazily created resources exist before the capture)
    eng.flush()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        eng.transition(fd, md, v)
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    eng.flush()
    assert torch.equal(v, v_plain) and float(v.abs().max()) > 0.0
    sc = eng.scalars()
    assert sc['data_term'] == sc_plain['data_term'] and sc['reg_energy'] == sc_plain['reg_energy'] and int(eng.state().iteration) == 4


# ------------------------------------------------------------------------------------------------------------------------------
# autograd: model.loss.NGF runs the two HIP operators in both directions
# ------------------------------------------------------------------------------------------------------------------------------
def test_autograd_of_the_loss_class():
    from ir_sgmcmc_amd.model.loss import DataLoss, NGF
    dims, Cn, w = (5, 6, 7), 2, 3.0
    loss = NGF(weight=w, fixed_eps=EPS[0], moving_eps=EPS[1])
    assert isinstance(loss, DataLoss) and loss.no_components == 1
    fixed, moving = N.images(dims, Cn)
    fixed = fixed[:1]
    wgt = N.upstream(dims, Cn)          # what sits between the map and the loss: any weights, negative ones too
    m = moving.to(DEV).requires_grad_(True)
    z = loss.map(fixed.to(DEV).expand(Cn, -1, -1, -1, -1), m)
    total = loss(z * wgt.to(DEV))
    total.backward()
    u = torch.tensor(w, dtype=torch.float32) * wgt      # the upstream gradient as the backward receives it, float32
    ref = N.reference(fixed, moving, u, *EPS)
    T = 'ngf/autograd'
    within(T, 'map', z, ref['d'].expand(Cn, -1, -1, -1, -1), ref['tol']['d'].expand(Cn, -1, -1, -1, -1))
    within(T, 'loss', total, ref['sums'].sum(), ref['tol']['sums'].sum())
    within(T, 'dL/dM', m.grad, ref['g'], ref['tol']['g'])
    same_bits(T, 'dL/dM against the float32 restatement', m.grad, N.restate32(fixed, moving, u, *EPS)['g'])
    # the masked form the VI stage uses: loss(map[mask]); and edge parameters left to the class
    mask = torch.rand(Cn, 1, *dims, generator=torch.Generator().manual_seed(4)) > 0.3
    m2 = moving.to(DEV).requires_grad_(True)
    loss(loss.map(fixed.to(DEV), m2)[mask.to(DEV)]).backward()
    ref2 = N.reference(fixed, moving, w * mask.to(F64), *EPS)
    within(T, 'dL/dM, masked', m2.grad, ref2['g'], ref2['tol']['g'])
    with pytest.raises(NotImplementedError, match='moving image only'):
        loss.map(fixed.to(DEV).requires_grad_(True), moving.to(DEV))
    auto = NGF(weight=1.0)
    found = ngf.ngf_edge_parameters(fixed, moving)
    assert torch.equal(auto.map(fixed.to(DEV), moving.to(DEV)), ngf.ngf_forward(fixed.to(DEV), moving.to(DEV), *found)['d'])


# ------------------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------------------
def refused(lib, cfg):
    ctx = C.c_void_p()
    assert lib.irs_create(C.byref(cfg), C.byref(ctx)) != 0 and not ctx.value
    return lib.irs_last_error().decode()


def test_refusals():
    lib = L.load()
    base = dict(dims=(16, 16, 16), data_loss='NGF', virtual_decimation=False)
    assert 'NGF data term takes no virtual decimation' in refused(lib, irs_config(EngineConfig(**{**base, 'virtual_decimation': True})))
    cfg = irs_config(EngineConfig(**base))
    cfg.data_loss = 2       # reserved
    assert refused(lib, cfg) == 'irs_create: unknown data loss'
    cfg.data_loss = 6
    assert refused(lib, cfg) == 'irs_create: unknown data loss'
    # z-slabs: the library and the Python owner, with the same words
    cfg, ctx, scfg = irs_config(EngineConfig(**base)), C.c_void_p(), L.IrsSlabConfig(0, 0)
    assert lib.irs_slab_create(C.byref(cfg), C.byref(scfg), None, C.byref(ctx)) != 0 and not ctx.value
    msg = lib.irs_last_error().decode()
    assert 'irs_slab_create' in msg and 'NGF' in msg, msg
    from ir_sgmcmc_amd.slab import SlabEngine
    with pytest.raises(L.IrsError) as err:
        SlabEngine(EngineConfig(**base), DEV)
    assert str(err.value) == msg


def test_ngf_set_refusals():
    fixed, moving = pair24()
    zero = lambda: torch.zeros(1, 3, 24, 24, 24, device=DEV)
    # a context that never had irs_ngf_set refuses its first transition: no eps is guessed
    eng = TransitionEngine(EngineConfig(dims=(24, 24, 24), data_loss='NGF', virtual_decimation=False), DEV)
    fd, md = eng.prepare(fixed, moving)
    with pytest.raises(L.IrsError, match='needs irs_ngf_set'):
        eng.transition(fd, md, zero())
    for w, ef, em in ((0.0, 0.1, 0.1), (float('nan'), 0.1, 0.1), (1.0, 0.0, 0.1), (1.0, 0.1, -1.0), (1.0, float('inf'), 0.1), (1.0, 0.1, float('nan'))):
        with pytest.raises(L.IrsError, match='finite values > 0'):
            eng.ngf_set(w, ef, em)
    eng.ngf_set(2.0, 0.02, 0.03)     # before the first transition: fine, and then it runs
    eng.transition(fd, md, zero())
    eng.flush()
    assert math.isfinite(eng.scalars()['data_term'][0]) and eng.scalars()['data_term'][0] > 0.0
    with pytest.raises(L.IrsError, match='only before the first transition'):
        eng.ngf_set(2.0, 0.02, 0.03)
    other = TransitionEngine(EngineConfig(dims=(24, 24, 24), data_loss='SSD', virtual_decimation=False), DEV)
    with pytest.raises(L.IrsError, match='not IRS_DATA_NGF'):
        other.ngf_set(1.0, 0.1, 0.1)
    with pytest.raises(L.IrsError, match='finite values > 0'):
        ngf24(1, ngf_weight=0.0)


# ------------------------------------------------------------------------------------------------------------------------------
# the trainer: the new config cut to 16^3 and ten transitions
# ------------------------------------------------------------------------------------------------------------------------------
def make_trainer(tmp_path, top=None, **trainer_over):
    from ir_sgmcmc_amd.parse_config import ConfigParser
    from ir_sgmcmc_amd.trainer import Trainer
    cfg = json.load(open(os.path.join(ROOT, 'configs', 'synthetic_ngf_l2_128.json')))
    cfg['trainer']['save_dir'] = str(tmp_path)
    cfg['data_loader']['args']['dims'] = [16, 16, 16]
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
    from ir_sgmcmc_amd.data_loader import synthetic_pair
    a = make_trainer(tmp_path / 'a')
    torch.manual_seed(0)
    a.run()
    a.engine.flush()
    ec = a.engine.cfg
    cfg = json.load(open(os.path.join(ROOT, 'configs', 'synthetic_ngf_l2_128.json')))['data_loss']['args']
    # the null edge parameters were computed once from the pair: the fixed image under its mask, the moving image under its own
    f1, m1 = synthetic_pair((16, 16, 16), seed=0, moving_contrast='invert', moving_bias=0.5)
    want = ngf.ngf_edge_parameters(f1['im'].unsqueeze(0), m1['im'].unsqueeze(0), f1['mask'].unsqueeze(0), m1['mask'].unsqueeze(0))
    assert (ec.data_loss, ec.ngf_weight) == ('NGF', cfg['weight']) and cfg['fixed_eps'] is None and cfg['moving_eps'] is None
    assert ec.ngf_fixed_eps == pytest.approx(want[0], rel=1e-6) and ec.ngf_moving_eps == pytest.approx(want[1], rel=1e-6)
    assert bool(torch.isfinite(a.v_curr_state).all()) and float(a.v_curr_state.abs().max()) > 0.0
    res = a.metrics.result()
    assert math.isfinite(res['MCMC/chain_0/data_term']) and res['MCMC/chain_0/data_term'] > 0.0
    # the data term the trainer logs is weight * sum mask d of the last warped image
    out = ngf.ngf_forward(a._fixed['im'], a._outputs['im_moving_warped'], ec.ngf_fixed_eps, ec.ngf_moving_eps, a._fixed['mask'].to(torch.float32))
    within('ngf/trainer', 'data_term of the last transition', a.engine.scalars()['data_term'], ec.ngf_weight * out['sums'],
           1e-5 * ec.ngf_weight * out['sums'].abs())
    ck = a.config.save_dirs['checkpoints'] / 'checkpoint_0000004.pt'
    assert ck.is_file()
    b = make_trainer(tmp_path / 'b', resume=str(ck))
    torch.manual_seed(0)
    b.run()
    assert all(torch.equal(x, z) if isinstance(x, torch.Tensor) else x == z for x, z in zip(digest(a), digest(b)))


def test_trainer_vi_stage_runs_with_the_class(tmp_path):
    t = make_trainer(tmp_path, VI=True, MCMC=False, no_iters_VI=2, no_samples_VI_test=1, log_period_VI=1)
    t.run()
    res = t.metrics.result()
    assert t.metrics._count['VI/train/data_term'] == 2 and math.isfinite(res['VI/train/data_term']) and res['VI/train/data_term'] > 0.0
    assert math.isfinite(res['VI/train/total_loss'])
    # the config's nulls stay null; the VI stage ran with the two values found for this pair, the engine's
    dl = t.losses['data']['loss']
    assert dl.fixed_eps is None and dl.moving_eps is None and dl.found_eps == (t.engine.cfg.ngf_fixed_eps, t.engine.cfg.ngf_moving_eps)


def test_trainer_refusals(tmp_path):
    with pytest.raises(ValueError, match='virtual decimation'):
        make_trainer(tmp_path / 'a', top={'virtual_decimation': True})._engine_config()
    with pytest.raises(ValueError, match='residual_check'):
        make_trainer(tmp_path / 'b', residual_check={'bins': 32})._engine_config()


# ------------------------------------------------------------------------------------------------------------------------------
# behaviour: a noise-free chain on the inverted, biased pair lowers its own data term
# ------------------------------------------------------------------------------------------------------------------------------
BEHAVIOUR = dict(dims=(32, 32, 32), lr=0.4, weight=1.0, transitions=40)


def test_noise_free_chain_lowers_its_data_term():
    """32^3, moving_contrast "invert", moving_bias 0.5, seed 0; 40 transitions with injected zero noise, jitter off, lr 0.4, weight 1,
    edge parameters by ngf_edge_parameters, the defaults of EngineConfig otherwise.  Only the chain's own data term is asserted."""
    from ir_sgmcmc_amd.data_loader import synthetic_pair
    dims = BEHAVIOUR['dims']
    f1, m1 = synthetic_pair(dims, seed=0, moving_contrast='invert', moving_bias=0.5)
    fixed = to_dev({k: v.unsqueeze(0) for k, v in f1.items() if k != 'seg'})
    moving = to_dev({k: v.unsqueeze(0) for k, v in m1.items() if k != 'seg'})
    eps = ngf.ngf_edge_parameters(fixed['im'], moving['im'], fixed['mask'], moving['mask'])
    eng = TransitionEngine(EngineConfig(dims=dims, data_loss='NGF', virtual_decimation=False, uniform_noise=0.0, lr=BEHAVIOUR['lr'],
                                        ngf_weight=BEHAVIOUR['weight'], ngf_fixed_eps=eps[0], ngf_moving_eps=eps[1]), DEV)
    fd, md = eng.prepare(fixed, moving)
    v, zero = torch.zeros(1, 3, *dims, device=DEV), torch.zeros(1, 3, *dims, device=DEV)
    terms = []
    for _ in range(BEHAVIOUR['transitions']):
        eng.transition(fd, md, v, None, zero, None)
        terms.append(eng.scalars()['data_term'][0])
    print(f'ngf/behaviour: data term {terms[0]:.6g} -> {terms[-1]:.6g} over {len(terms)} transitions, eps {eps[0]:.4g} / {eps[1]:.4g}')
    assert terms[-1] < terms[0]
