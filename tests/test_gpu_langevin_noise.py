"""The in-kernel Langevin noise -- perturb_kernel (csrc/field_kernels.hip) and perturb_sobolev_march_kernel (csrc/stencil_kernels.hip)
with eps = NULL, what every production run draws -- element by element against the integer restatement of tests/_langevin_noise.py
(proved on the CPU by tests/test_langevin_noise_host.py): Philox4x32-10 counters and key, split21, the assignment of the six normals
of a voxel pair, Box-Muller within `tol(r)`, the edge words, the combine bit for bit, the fused kernel against the two-kernel form
with identity taps, and the seed / iteration an engine with several chains hands to either kernel.

Shapes: (5,6,70) x 3 chains (odd D: the last pair is half written; H no multiple of the 4-row block; W a 64 block plus 6), (4,8,64) x 2
(exact block multiples), (2,2,2) x 2 (the smallest volume irs_perturb_smooth accepts -- D = 1 is refused, asserted below --: one pair)."""
import math

import pytest
import torch

from ir_sgmcmc_amd import _lib as L
from ir_sgmcmc_amd import ops
from ir_sgmcmc_amd.engine import EngineConfig, TransitionEngine
from tests import _langevin_noise as N
from tests._report import check

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F64 = torch.float64

SHAPES = [((5, 6, 70), 3), ((4, 8, 64), 2), ((2, 2, 2), 2)]
IDS = ['x'.join(map(str, d)) + f'-C{c}' for d, c in SHAPES]
ITERATIONS = (0, 7, 2 ** 32 + 7)
SEEDS = (5, 5 + 2 ** 32)


def check_each(test, key, a, b, tol):
    """|a - b| <= tol element by element; the parity report gets the worst deviation in units of its tolerance"""
    a, b, tol = (torch.as_tensor(x, dtype=F64).cpu() for x in (a, b, tol))
    return check(test, key + ' [deviation / tolerance]', torch.where(a == b, torch.zeros_like(tol), (a - b).abs() / tol), torch.zeros_like(tol), 1.0)


def drawn(C, dims, seed, iteration):
    """the normals the two-kernel form draws: v = 0, amp = sqrt(2 * 0.5) = 1, no sigma -> 0 + (1 * 1) * n = n"""
    return ops.perturb_smooth(torch.zeros(C, 3, *dims, device=DEV), None, tau=0.5, seed=seed, iteration=iteration)


# ---------------------------------------------------------------- noise per element
@pytest.mark.parametrize('dims,C', SHAPES, ids=IDS)
def test_noise_element_by_element(dims, C):
    T = 'langevin_noise/' + 'x'.join(map(str, dims)) + f'-C{C}'
    for seed in SEEDS:
        for it in ITERATIONS:
            ref, r = N.normals(seed, it, C, dims)
            out = drawn(C, dims, seed, it).cpu()
            assert bool(torch.isfinite(out).all())
            ratio = check_each(T, f'seed {seed} iteration {it}', out, ref, N.tol(r))
            print(f'{T}: seed {seed} iteration {it}: worst deviation / tolerance {ratio:.4f}')


def test_a_single_plane_is_refused():
    with pytest.raises(L.IrsError):
        drawn(2, (1, 2, 2), 5, 0)


# ---------------------------------------------------------------- edges
def edge_call(edge):
    it, c, vox, ch = edge
    other = N.partner(N.EDGE_DIMS, vox, ch)
    out = drawn(N.EDGE_CHAINS, N.EDGE_DIMS, N.EDGE_SEED, it).cpu()
    ref, r = N.normals(N.EDGE_SEED, it, N.EDGE_CHAINS, N.EDGE_DIMS)
    assert bool(torch.isfinite(out).all())
    at, at2 = (c, ch) + vox, (c, other[1]) + other[0]
    return float(out[at]), float(out[at2]), float(ref[at]), float(ref[at2]), float(r[at])


def test_edge_words():
    T = 'langevin_noise/edge_words'
    # a = 0: the 5.4-sigma tail, finite and inside the largest radius
    n0, n1, ref0, ref1, r = edge_call(N.EDGE_A_MIN)
    assert abs(r - N.R_MAX) < 1e-12
    assert abs(n0) <= N.R_MAX and abs(n1) <= N.R_MAX
    check_each(T, 'a = 0', [n0, n1], [ref0, ref1], [N.tol(r)] * 2)
    # a = 2^21 - 1: u = 1, the radius is 0
    n0, n1, ref0, ref1, r = edge_call(N.EDGE_A_MAX)
    assert r == 0.0 and ref0 == 0.0 and ref1 == 0.0
    check_each(T, 'a = 2^21 - 1', [n0, n1], [ref0, ref1], [N.tol(r)] * 2)
    # b = 0: angle 0, the sin element exactly 0 and the cos element the radius itself
    n0, n1, ref0, ref1, r = edge_call(N.EDGE_B_ZERO)
    assert ref0 == r and ref1 == 0.0
    assert n1 == 0.0
    check_each(T, 'b = 0', [n0], [r], [N.tol(r)])


# ---------------------------------------------------------------- the combine, bit for bit
@pytest.mark.parametrize('dims,C', SHAPES, ids=IDS)
def test_combine_bit_for_bit(dims, C):
    """out = v + (amp * sigma) * n with one float32 rounding per operation (__fmul_rn / __fadd_rn: nothing contracts), amp = sqrtf(2 tau)"""
    g = torch.Generator().manual_seed(3)
    v = torch.randn(C, 3, *dims, generator=g)
    sigma = torch.rand(C, 3, *dims, generator=g) + 0.25
    n = drawn(C, dims, 5, 7).cpu()
    # sqrtf(2.0f * tau): the float32 product, its square root taken in double and rounded once (53 >= 2 * 24 + 2 bits: the same as a
    # correctly rounded float32 root, which a vectorised float32 sqrt of the CPU need not be)
    amp = torch.tensor(math.sqrt(float(torch.tensor(2.0, dtype=torch.float32) * torch.tensor(0.4, dtype=torch.float32))), dtype=torch.float32)
    out = ops.perturb_smooth(v.to(DEV), None, sigma.to(DEV), tau=0.4, seed=5, iteration=7).cpu()
    assert torch.equal(out, v + (amp * sigma) * n)
    out = ops.perturb_smooth(v.to(DEV), None, tau=0.4, seed=5, iteration=7).cpu()
    assert torch.equal(out, v + (amp * torch.ones_like(sigma)) * n)


# ---------------------------------------------------------------- the fused kernel on its own
@pytest.mark.parametrize('dims,C', SHAPES, ids=IDS)
def test_fused_kernel_with_identity_taps_draws_the_same_field(dims, C):
    """taps [0, 1, 0]: s = 1 and a smoothing that is the identity (fma(0, x, 0) = 0, fma(1, x, 0) = x, fma(0, y, x) = x), so the fused
    kernel's output is its perturbed field: every generated normal of every tile -- halos and the stashed odd plane included, which
    the smoothing then discards or passes on -- against the two-kernel perturbation, which test_noise_element_by_element holds to the
    restatement"""
    g = torch.Generator().manual_seed(4)
    v = torch.randn(C, 3, *dims, generator=g).to(DEV)
    sigma = (torch.rand(C, 3, *dims, generator=g) + 0.25).to(DEV)
    zeros = torch.zeros_like(v)
    ident = [0.0, 1.0, 0.0]
    try:
        for seed, it in ((5, 7), (5 + 2 ** 32, 2 ** 32 + 7)):
            plain = drawn(C, dims, seed, it)
            with_sigma = ops.perturb_smooth(v, None, sigma, tau=0.5, seed=seed, iteration=it)
            assert not torch.equal(plain, zeros)
            for rows in (0, 16, 32):
                L.option_set('fuse_noise', 1)
                L.option_set('ps_rows', rows)
                assert torch.equal(ops.perturb_smooth(zeros, ident, tau=0.5, seed=seed, iteration=it), plain), (rows, seed, it)
                assert torch.equal(ops.perturb_smooth(v, ident, sigma, tau=0.5, seed=seed, iteration=it), with_sigma), (rows, seed, it, 'sigma')
    finally:
        L.option_set('fuse_noise', 1)
        L.option_set('ps_rows', 0)


# ---------------------------------------------------------------- engine plumbing, several chains
@pytest.mark.parametrize('sobolev_s', [0, 1], ids=['two_kernel', 'fused'])
def test_engine_hands_seed_and_iteration_to_the_kernel(sobolev_s):
    """transition k of an engine perturbs (and, sobolev_s = 1, smooths in the fused kernel, the iteration read from the device) with
    (seed, iteration k): its `curr_state` is the stateless operator's output on the velocity it started from, for every chain"""
    dims, C, seed = (9, 10, 70), 3, 11
    cfg = EngineConfig(dims=dims, no_chains=C, sobolev_s=sobolev_s, lr=0.5, uniform_noise=0.0, data_loss='SSD', seed=seed)
    kernel = ops.sobolev_kernel_1d(sobolev_s, cfg.sobolev_lambda) if sobolev_s else None
    g = torch.Generator().manual_seed(6)
    fixed = {'im': torch.rand(1, 1, *dims, generator=g).to(DEV), 'mask': torch.ones(1, 1, *dims, dtype=torch.bool, device=DEV)}
    moving = {'im': torch.rand(1, 1, *dims, generator=g).to(DEV)}
    eng = TransitionEngine(cfg, DEV)
    fd, md = eng.prepare(fixed, moving)
    v = torch.zeros(C, 3, *dims, device=DEV)
    out = {'curr_state': torch.full((C, 3, *dims), float('nan'), device=DEV)}
    for start in (0, 2 ** 32 + 3):
        if start:
            st = eng.state()
            st.iteration = start
            eng.set_state(st)
        assert eng.state().iteration == start
        for k in range(start, start + 3):
            before = v.clone()
            eng.transition(fd, md, v, outputs=out)
            assert eng.state().iteration == k + 1          # (state() waits for the transition)
            cs = out['curr_state']
            assert torch.equal(cs, ops.perturb_smooth(before, kernel, tau=0.5, seed=seed, iteration=k)), (start, k)
            assert not torch.equal(cs, ops.perturb_smooth(before, kernel, tau=0.5, seed=seed, iteration=k + 1))
            noise = cs - before if not sobolev_s else cs
            for a, b in ((0, 1), (0, 2), (1, 2)):                # (at k = 0 every chain starts from the same v = 0)
                assert float((noise[a] == noise[b]).float().mean()) < 0.01, (a, b)
            assert bool(torch.isfinite(v).all())
