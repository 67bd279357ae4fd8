"""irs_ffd_up / irs_ffd_adjoint (ffd_axis_kernel, csrc/field_kernels.hip) per element: against the float64 matrix form of
tests/_ffd.py within the bounds derived there, bit for bit on impulses (exact zeros off the support included), as an adjoint pair,
with a scratch of exactly irs_ffd_scratch_floats floats in front of a guard, and through the modules of utils/transformation.py.
tests/test_ffd_host.py holds the reference side to the oracle on the CPU.  Every launch is a volume of a few thousand voxels.  GPU only."""
import ctypes as C

import pytest
import torch

from ir_sgmcmc_amd import _lib as L
from ir_sgmcmc_amd import ops as G
from ir_sgmcmc_amd.utils.transformation import SVF_3D, SVFFD_3D, Cubic_B_spline_FFD_3D
from tests import _ffd as F

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CASES = pytest.mark.parametrize('dims,cps', F.CASES, ids=F.IDS)
SENTINEL = 0x7FA5C3E1  # a NaN no kernel here computes

_RUNS = {}


def dev(t):
    return t.to(DEV).contiguous()


def scratch_is_sized(Cn, dims, cps):
    """the wrappers allocate what irs_ffd_scratch_floats says: a wrong answer is a failed assertion here, before any launch"""
    n = L.load().irs_ffd_scratch_floats(Cn, *dims, *cps)
    assert n == F.scratch_floats(Cn, dims, cps), (n, F.scratch_floats(Cn, dims, cps))
    return n


def up(v, dims, cps):
    scratch_is_sized(v.shape[0], dims, cps)
    return G.ffd_up(dev(v), dims, cps).cpu()


def adjoint(g, cps):
    scratch_is_sized(g.shape[0], tuple(g.shape[2:]), cps)
    return G.ffd_adjoint(dev(g), cps).cpu()


def run(dims, cps, Cn):
    """inputs, device outputs, float64 references and bounds of a case: computed once, shared, never modified"""
    key = (dims, cps, Cn)
    if key not in _RUNS:
        v, g = F.inputs(dims, cps, Cn)
        _RUNS[key] = dict(v=v, g=g, up=up(v, dims, cps), adj=adjoint(g, cps), up64=F.up64(v, dims, cps), adj64=F.adj64(g, cps),
                          up_bound=F.up_bound(v, dims, cps), adj_bound=F.adj_bound(g, cps))
    return _RUNS[key]


def assert_within(what, out, ref, bound):
    assert out.dtype == torch.float32 and out.shape == ref.shape, (what, out.dtype, tuple(out.shape), tuple(ref.shape))
    err = (out.double() - ref).abs()
    bad = (~(err <= bound)).nonzero()  # a NaN is beyond every bound
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f'{what}: worst error {worst:.3f} of its bound')
    first = [(tuple(int(i) for i in ix), out[tuple(ix)].item(), ref[tuple(ix)].item(), bound[tuple(ix)].item()) for ix in bad[:6]]
    assert len(bad) == 0, f'{what}: {len(bad)} of {out.numel()} elements beyond their bound; first (index, got, float64, bound): {first}'


def assert_bits(what, out, ref):
    """equal as bit patterns (+0 is not -0), the differing elements located"""
    assert out.dtype == ref.dtype == torch.float32 and out.shape == ref.shape, (what, out.dtype, tuple(out.shape), tuple(ref.shape))
    a, b = out.contiguous().view(torch.int32), ref.contiguous().view(torch.int32)
    if torch.equal(a, b):
        return
    bad = (a != b).nonzero()
    first = [(tuple(int(i) for i in ix), out[tuple(ix)].item(), ref[tuple(ix)].item()) for ix in bad[:8]]
    raise AssertionError(f'{what}: {len(bad)} of {out.numel()} elements differ; first (index, got, expected): {first}')


# ---------------------------------------------------------------- 1. element by element against float64
@pytest.mark.parametrize('Cn', [1, 3])
@CASES
def test_up_and_adjoint_per_element(dims, cps, Cn):
    r = run(dims, cps, Cn)
    assert_within(f'ffd_up {dims} / {cps}', r['up'], r['up64'], r['up_bound'])
    assert_within(f'ffd_adjoint {dims} / {cps}', r['adj'], r['adj64'], r['adj_bound'])


# ---------------------------------------------------------------- 2. control-grid impulses
@pytest.mark.parametrize('a', [1.0, 2.0 ** 100], ids=['1', '2^100'])
@CASES
def test_control_impulses_bit_for_bit(dims, cps, a):
    """nine impulses a launch, one per (chain, channel), over the product of j in {0, 3, interior, G - 1} per axis"""
    for pos in F.batches(F.control_picks(dims, cps)):
        out = up(F.impulses(F.grid(dims, cps), pos, a), dims, cps)
        assert_bits(f'ffd_up of {a} at {pos}, {dims} / {cps}', out, F.expected_up(dims, cps, pos, a))


# ---------------------------------------------------------------- 3. dense impulses through the adjoint
@pytest.mark.parametrize('a', [1.0, 2.0 ** 100], ids=['1', '2^100'])
@CASES
def test_dense_impulses_bit_for_bit(dims, cps, a):
    """x in {0, c - 1, c, N - 1} per axis, clamped to the volume"""
    for pos in F.batches(F.dense_picks(dims, cps)):
        out = adjoint(F.impulses(dims, pos, a), cps)
        assert_bits(f'ffd_adjoint of {a} at {pos}, {dims} / {cps}', out, F.expected_adj(dims, cps, pos, a))


# ---------------------------------------------------------------- 4. adjointness
@CASES
def test_adjointness(dims, cps):
    """<up(v), g> = <v, adj(g)> from the device outputs, summed in float64, within the two element bounds summed the same way"""
    r = run(dims, cps, 3)
    v, g = r['v'].double(), r['g'].double()
    lhs, rhs = float((r['up'].double() * g).sum()), float((v * r['adj'].double()).sum())
    tol = float((r['up_bound'] * g.abs()).sum() + (v.abs() * r['adj_bound']).sum())
    print(f'<up v, g> - <v, adj g> = {lhs - rhs:.3e}, tolerance {tol:.3e}')
    assert abs(lhs - rhs) <= tol


# ---------------------------------------------------------------- 5. the scratch contract
@CASES
def test_scratch_contract(dims, cps):
    """The C entry points with a scratch of exactly irs_ffd_scratch_floats floats, followed in the same allocation by a guard of
    sentinel words at least as long as what 2 x (C,3,D,H,W) falls short of the two intermediates (so a library sized by that
    older rule writes into the guard and nowhere else): the guard stays untouched, the results are the wrappers'."""
    Cn = 3
    lib, st = L.load(), L.stream_ptr()
    n, need = lib.irs_ffd_scratch_floats(Cn, *dims, *cps), F.scratch_floats(Cn, dims, cps)
    shortfall = max(need - F.old_contract_floats(Cn, dims), 0)
    guard = max(shortfall, need - n, 0) + 64
    v, g = F.inputs(dims, cps, Cn, seed=1)
    v_d, g_d = dev(v), dev(g)
    results = []
    for fn, src, shape in ((lib.irs_ffd_up, v_d, (Cn, 3, *dims)), (lib.irs_ffd_adjoint, g_d, (Cn, 3, *F.grid(dims, cps)))):
        buf = torch.full((n + guard,), SENTINEL, dtype=torch.int32, device=DEV)
        out = torch.empty(shape, device=DEV, dtype=torch.float32)
        L.check(fn(L.dev_ptr(src), L.dev_ptr(out), C.c_void_p(buf.data_ptr()), Cn, *dims, *cps, st))
        torch.cuda.synchronize()
        touched = (buf[n:].cpu() != SENTINEL).nonzero().flatten()
        assert len(touched) == 0, (f'{fn.__name__}: {len(touched)} words behind the {n} floats of scratch overwritten, the first at '
                                   f'+{int(touched[0])}, the last at +{int(touched[-1])} (shortfall of 2 x (C,3,D,H,W): {shortfall})')
        results.append(out.cpu())
    assert n == need
    assert_bits('irs_ffd_up against ops.ffd_up', results[0], up(v, dims, cps))
    assert_bits('irs_ffd_adjoint against ops.ffd_adjoint', results[1], adjoint(g, cps))


# ---------------------------------------------------------------- 6. the modules
def test_modules_at_cps_1_2_1():
    dims, cps, Cn = (6, 7, 9), (1, 2, 1), 2
    scratch_is_sized(Cn, dims, cps)
    v, g = F.inputs(dims, cps, Cn, seed=2)
    v_d, g_d = dev(v).requires_grad_(True), dev(g)
    out = Cubic_B_spline_FFD_3D(dims, cps)(v_d)
    out.backward(g_d)
    dense = G.ffd_up(v_d.detach(), dims, cps)
    assert_bits('Cubic_B_spline_FFD_3D.forward', out.detach().cpu(), dense.cpu())
    assert_bits('Cubic_B_spline_FFD_3D backward', v_d.grad.cpu(), G.ffd_adjoint(g_d, cps).cpu())
    assert_within('ffd_up (6,7,9) / (1,2,1)', dense.cpu(), F.up64(v, dims, cps), F.up_bound(v, dims, cps))
    small = dev(torch.randn(Cn, 3, *F.grid(dims, cps), generator=torch.Generator().manual_seed(7)))  # a velocity of about a voxel
    t, d = SVFFD_3D(dims, cps)(small)
    t_ref, d_ref = SVF_3D(dims)(G.ffd_up(small, dims, cps))
    assert_bits('SVFFD_3D transformation', t.cpu(), t_ref.cpu())
    assert_bits('SVFFD_3D displacement', d.cpu(), d_ref.cpu())
