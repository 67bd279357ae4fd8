"""The warp family held bit for bit to the fp64 reference on the exact ("dyadic") cases of tests/_exact_cases.py (DESIGN.md,
"Numerics": the exact-case method): trilinear forward / adjoint, nearest, shared and per-chain images; the in-kernel Philox
jitter against its integer restatement and against statistics that do not go through it; the warp inside a transition of the
engine (iteration read from the device state, gradient written for the adjoint) pinned to the same counter layout; the LCC map
with a per-chain fixed image.  GPU only."""
import math

import pytest
import torch

from ir_sgmcmc_amd import ops as G
from oracle import ops as O
from tests import _exact_cases as X
from tests._report import check
from tests.test_gpu_ops import dev, smooth_field

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def assert_same(what, out, ref):
    """torch.equal with the failing elements located: how many, which chains / axes, the first few (index, got, expected)"""
    out, ref = out.cpu(), ref.to(out.dtype) if not ref.dtype.is_floating_point else ref.float()
    assert out.shape == ref.shape, (what, tuple(out.shape), tuple(ref.shape))
    if torch.equal(out, ref):
        return
    bad = (out != ref).nonzero()
    first = [(tuple(int(i) for i in ix), out[tuple(ix)].item(), ref[tuple(ix)].item()) for ix in bad[:8]]
    per_chain = torch.bincount(bad[:, 0], minlength=out.shape[0]).tolist()
    per_channel = torch.bincount(bad[:, 1], minlength=out.shape[1]).tolist()
    raise AssertionError(f'{what}: {len(bad)} of {out.numel()} elements differ; per chain {per_chain}, per channel {per_channel}, '
                         f'x-blocks {sorted(set((bad[:, -1] // 64).tolist()))}; first (index, got, expected): {first}')


# ---------------------------------------------------------------- trilinear: value, explicit transformation, adjoint
_REF = {}


def _reference(dims, per_chain, jitter):
    """fp64 reference of a case, computed once and shared (never modified)"""
    key = (tuple(dims), per_chain, jitter)
    if key not in _REF:
        case = X.warp_case(dims, per_chain)
        _REF[key] = (case,) + X.warp_reference(case, torch.float64, jitter)
    return _REF[key]


@pytest.mark.parametrize('jitter', [False, True])
@pytest.mark.parametrize('dims,per_chain', X.WARP_CASES)
def test_trilinear_warp_and_adjoint_are_exact(dims, per_chain, jitter):
    """Value, value on the explicit transformation, and grid gradient, torch.equal to fp64.  What the border mask of axis_tap does
    shows at the LOWER border (coordinate exactly 0: taps 0 and 1, weight 1 on the first, gradient forced to 0).  At the upper
    border (exactly n - 1) both taps are the clamped last voxel, the signed tap sum is exactly 0 and the mask cannot be seen."""
    case, out64, gd64, grid64 = _reference(dims, per_chain, jitter)
    im, d, gw = dev(case.im), dev(case.d_last), dev(case.g_warped)
    unif, alpha = (dev(case.unif), case.alpha) if jitter else (None, 0.0)
    assert_same('warp_displacement', G.warp_displacement(im, d, unif, alpha), out64)
    assert_same('warp on the transformation', G.warp(im, dev(grid64.float())), out64)
    assert_same('warp_displacement_bwd', G.warp_displacement_bwd(im, d, gw, unif, alpha), gd64)


# ---------------------------------------------------------------- nearest
@pytest.mark.parametrize('dims', X.EXACT_DIMS)
def test_nearest_warp_is_exact_on_ties_and_outside(dims):
    case = X.nearest_case(dims)
    t = dev(case.transformation)
    for name in ('labels_shared', 'labels_chain', 'mask_shared', 'mask_chain'):
        seg = getattr(case, name)
        out = G.warp(dev(seg), t)
        assert out.dtype == seg.dtype
        assert_same(name, out, X.nearest_reference(seg, case.transformation, torch.float64))


# ---------------------------------------------------------------- in-kernel jitter against the integer restatement
def _jitter_inputs(dims, exact):
    if exact:
        case = X.warp_case(dims, True)
        return case.im, case.d_last, case.g_warped, 0.5
    g = torch.Generator().manual_seed(17)
    C = X.CHAINS
    im = torch.rand(1, 1, *dims, generator=g)
    # one displacement for all chains: whatever differs between the chains is the jitter
    d = (smooth_field(1, dims, 4.0, 18) * (2.0 / (min(dims) - 1))).expand(C, -1, -1, -1, -1).contiguous()
    return im, d, torch.randn(C, 1, *dims, generator=g), 0.4


@pytest.mark.parametrize('seed,iteration', [(0, 0), (5, 7), (5, 2 ** 28 + 3)])
@pytest.mark.parametrize('dims,exact', [((9, 17, 33), True), ((7, 13, 70), False)])
def test_in_kernel_jitter_draws_what_the_restatement_draws(dims, exact, seed, iteration):
    """Downstream of u both branches of jitter_point run the same expressions, so the warp with in-kernel draws and the warp given
    the restated draws are bit-identical -- forward and adjoint -- if and only if counter, key and bit splitting are the stated ones."""
    im, d, gw, alpha = _jitter_inputs(dims, exact)
    C = d.shape[0]
    u = X.philox_jitter_uniforms(seed, iteration, C, dims)
    im_d, d_d, gw_d, u_d = dev(im), dev(d), dev(gw), dev(u)
    fwd = G.warp_displacement(im_d, d_d, None, alpha, seed, iteration)
    assert_same('forward', fwd, G.warp_displacement(im_d, d_d, u_d, alpha).cpu())
    bwd = G.warp_displacement_bwd(im_d, d_d, gw_d, None, alpha, seed, iteration)
    assert_same('adjoint', bwd, G.warp_displacement_bwd(im_d, d_d, gw_d, u_d, alpha).cpu())
    assert not torch.equal(u[0], u[1]) and not torch.equal(u[0], u[2])
    if not exact:   # same image, same displacement: the chains differ by their draws alone
        assert not torch.equal(fwd[1], fwd[0]) and not torch.equal(fwd[2], fwd[0])
        assert not torch.equal(bwd[1], bwd[0]) and not torch.equal(bwd[2], bwd[0])
    assert not torch.equal(fwd, G.warp_displacement(im_d, d_d, None, alpha, seed, iteration + 1))


# ---------------------------------------------------------------- the draws themselves, without the restatement
def test_in_kernel_jitter_draws_are_uniform_and_independent():
    """Warp the three ramp images (value = x, y, z index) with d = 0 and in-kernel jitter: in the interior the warped ramp is the
    sampling coordinate, so offset = warped - index = alpha - 2 alpha u gives u back.  Same form as test_philox_noise_statistics.
    The recovered u carries the fp32 rounding of the coordinate arithmetic and of the 8-tap sum: with n - 1 <= 35, each of
    id + jitter, g + 1 and the product with n - 1 rounds a coordinate <= 35 voxels once (3 u 35), the eight products of three
    weights and a value <= 35 and their seven additions at most 3 + 7 more (10 u 35), u = 2^-24: |error| <= 13 * 2^-24 * 35
    voxels, E below in units of u.  [0, 1) is asserted up to that E; the moments are held to 5 standard errors."""
    dims, C, alpha = (20, 24, 36), 3, 0.5
    zero = torch.zeros(C, 3, *dims, device=DEV)
    z, y, x = torch.meshgrid(*(torch.arange(n, dtype=torch.float32) for n in dims), indexing='ij')
    inner = (slice(None), 0, slice(1, -1), slice(1, -1), slice(1, -1))
    us = []
    for ramp in (x, y, z):
        w = G.warp_displacement(dev(ramp.reshape(1, 1, *dims)), zero, None, alpha, 11, 4)
        off = (w.cpu().double() - ramp.double())[inner]
        us.append(((alpha - off) / (2.0 * alpha)).reshape(C, -1))
    u = torch.stack(us, 1)   # (C, 3, n)
    E = 13 * 2.0 ** -24 * 35 / (2.0 * alpha)
    assert float(u.min()) >= -E and float(u.max()) < 1.0 + E, (float(u.min()), float(u.max()))
    n = u.shape[-1]
    for c in range(C):
        for k in range(3):
            assert abs(float(u[c, k].mean()) - 0.5) < 5.0 * math.sqrt(1.0 / 12.0 / n), (c, k)
            assert abs(float(((u[c, k] - 0.5) ** 2).mean()) - 1.0 / 12.0) < 5.0 * math.sqrt(1.0 / 180.0 / n), (c, k)
    rows = (u - 0.5).reshape(C * 3, n) * math.sqrt(12.0)   # unit variance: the mean product of two rows is their correlation
    for a in range(C * 3):
        for b in range(a + 1, C * 3):   # components of one chain, and everything between chains
            assert abs(float((rows[a] * rows[b]).mean())) < 5.0 / math.sqrt(n), (divmod(a, 3), divmod(b, 3))
    # neighbours along x are independent draws too
    uv = (u[:, 0] - 0.5).reshape(C, dims[0] - 2, dims[1] - 2, dims[2] - 2) * math.sqrt(12.0)
    assert abs(float((uv[..., 1:] * uv[..., :-1]).mean())) < 5.0 / math.sqrt(uv[..., 1:].numel())


# ---------------------------------------------------------------- the warp inside a transition of the engine
def test_engine_jitter_is_the_same_counter_layout():
    """Two transitions with in-kernel jitter against the same two on a second engine given the restated draws.  The engine draws
    transition k (0-based, counted from its creation: gmm_init does not advance the counter, every completed transition does by
    one) with iteration k and the seed of its config, chain c at index c * D*H*W + voxel."""
    from ir_sgmcmc_amd.data_loader import synthetic_pair
    from ir_sgmcmc_amd.engine import EngineConfig, TransitionEngine
    dims, C, seed = (18, 26, 34), 2, 9
    f1, m1 = synthetic_pair(dims, seed=3)
    fixed = {k: dev(v.unsqueeze(0).expand(C, *v.shape)) for k, v in f1.items() if k != 'seg'}
    moving = {k: dev(v.unsqueeze(0).expand(C, *v.shape)) for k, v in m1.items() if k != 'seg'}
    g = torch.Generator().manual_seed(21)
    v0 = smooth_field(C, dims, 4.0, 22)
    eps = [torch.randn(C, 3, *dims, generator=g) for _ in range(2)]
    names = ('curr_state', 'im_moving_warped', 'residuals', 'displacement', 'transformation', 'grad_v')
    res = []
    for restated in (False, True):
        cfg = EngineConfig(dims=dims, no_chains=C, data_loss='GMM', uniform_noise=0.1, seed=seed)
        eng = TransitionEngine(cfg, DEV)
        fd, md = eng.prepare(fixed, moving)
        eng.gmm_init(fd, md)
        v = dev(v0)
        got = []
        for k in range(2):
            out = {n: torch.empty(C, 1 if n in ('im_moving_warped', 'residuals') else 3, *dims, device=DEV) for n in names}
            unif = dev(X.philox_jitter_uniforms(seed, k, C, dims)) if restated else None
            eng.transition(fd, md, v, None, dev(eps[k]), unif, out)
            eng.flush()
            got.append({**{n: t.clone() for n, t in out.items()}, 'v': v.clone()})
        assert eng.state().iteration == 2
        res.append(got)
    for k in range(2):
        for n in names + ('v',):
            assert bool(torch.isfinite(res[0][k][n]).all()), (k, n)
            assert_same(f'transition {k}: {n}', res[0][k][n], res[1][k][n].cpu())
    assert not torch.equal(res[0][0]['im_moving_warped'][0], res[0][0]['im_moving_warped'][1])


# ---------------------------------------------------------------- LCC map with a fixed image per chain
@pytest.mark.parametrize('dims', [(9, 8, 33), (12, 20, 40)])
@pytest.mark.parametrize('s', [1, 2])
def test_lcc_map_with_a_fixed_image_per_chain(dims, s):
    """irs_lcc_map_fwd / _bwd with Cf == C (fhat stride V); the tolerances of test_lcc_forward_backward: the same operation at the
    same sizes"""
    C = X.CHAINS
    g = torch.Generator().manual_seed(7)
    Fi = torch.rand(C, 1, *dims, generator=g)
    M = torch.rand(C, 1, *dims, generator=g).requires_grad_(True)
    T = f'lcc_per_chain/{"x".join(map(str, dims))}_s{s}'
    fhat = G.lcc_normalise(dev(Fi), s)
    check(T, 'fhat', fhat, O.lcc_normalise(Fi, s)[0], 2e-5)
    z_ref = O.lcc_map(Fi, M, s)
    z, sigm = G.lcc_map_fwd(fhat, dev(M.detach()), s)
    check(T, 'z', z, z_ref, 5e-5)
    gz = torch.randn(C, 1, *dims, generator=g)
    gref, = torch.autograd.grad(z_ref, M, gz)
    gout = G.lcc_map_bwd(fhat, z, sigm, dev(gz), s)
    gmax = float(gref.abs().max())
    check(T, 'g_warped (rel to max)', gout.cpu() / gmax, gref / gmax, 1e-4)
    # the chains' fixed images differ, so reading chain 0's for every chain cannot pass
    z0, _ = G.lcc_map_fwd(fhat[:1].contiguous(), dev(M.detach()), s)
    assert float((z0[1:] - z[1:]).abs().max()) > 1e-2
