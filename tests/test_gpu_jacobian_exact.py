"""irs_gradient_operator(transformation=1) and irs_log_det_jacobian against fp64: bit for bit on the exact ("dyadic")
transformations of tests/_exact_cases.py, where det J is exact in fp32 and takes every sign and the value 0; within derived
rounding bounds on smooth ragged fields ("Numerics": the exact-case method).  GPU only."""
import pytest
import torch

from ir_sgmcmc_amd import ops as G
from oracle import ops as O
from tests import _exact_cases as X
from tests._report import check
from tests.test_gpu_ops import dev, smooth_field

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U = 2.0 ** -24   # unit roundoff of fp32

_REF = {}


def _exact(dims):
    """(transformation fp32, nabla fp64, det fp64) of an exact case, computed once and shared (never modified)"""
    if dims not in _REF:
        t = X.transformation_case(dims)
        _REF[dims] = (t,) + X.jacobian_reference(t, torch.float64)
    return _REF[dims]


# ---------------------------------------------------------------- gradient operator
@pytest.mark.parametrize('dims', X.EXACT_DIMS)
def test_gradient_operator_of_a_transformation_is_exact(dims):
    t, nabla64, _ = _exact(dims)
    out = G.gradient_operator(dev(t), transformation=True).cpu()
    assert out.shape == nabla64.shape
    bad = (out != nabla64.float()).nonzero()
    assert len(bad) == 0, f'{len(bad)} elements differ; first (chain, axis, z, y, x, comp): {bad[:8].tolist()}'
    # the plain differences of the same field too (transformation=False leaves out the division)
    assert torch.equal(G.gradient_operator(dev(t)).cpu(), O.forward_differences(t.double()).float())


@pytest.mark.parametrize('dims', [(10, 14, 22), (7, 70, 13)])
def test_gradient_operator_of_a_transformation_on_ragged_fields(dims):
    """Per element 3 * 2^-24 |reference| -- one rounding each of the difference, of 2 / (n - 1) and of the division -- plus
    2^-24 max|t| (n - 1) / 2: what the rounding of the difference is relative to (its operands, not its small result)."""
    t, _ = O.svf_exp(smooth_field(2, dims, 6.0, 9))
    ref = O.forward_differences(t.double(), transformation=True)   # (C, 3 axes, D, H, W, 3)
    out = G.gradient_operator(dev(t.contiguous()), transformation=True).cpu().double()
    tmax = float(t.abs().max())
    T = f'gradient_operator_t/{"x".join(map(str, dims))}'
    for a, n in enumerate(X.axis_sizes(dims)):
        tol = 3 * U * ref[:, a].abs() + U * tmax * (n - 1) / 2.0
        check(T, f'd/d{"xyz"[a]} (in units of the bound)', (out[:, a] - ref[:, a]) / tol, torch.zeros_like(tol), 1.0)
    assert float(ref.abs().max()) > 0.5


# ---------------------------------------------------------------- log det J, exact
@pytest.mark.parametrize('dims', X.EXACT_DIMS)
def test_log_det_jacobian_on_exact_determinants(dims):
    t, _, det = _exact(dims)
    C = t.shape[0]
    t_d = dev(t)
    cnt, ld = G.log_det_jacobian(t_d)
    ld = ld.cpu()
    neg, zero, pos = det < 0, det == 0, det > 0
    assert torch.equal(torch.isnan(ld), neg), (int(torch.isnan(ld).sum()), int(neg.sum()))
    assert torch.equal(ld == -float('inf'), zero), (int((ld == -float('inf')).sum()), int(zero.sum()))
    assert bool(torch.isfinite(ld[pos]).all())
    ref = det[pos].log()
    tol = 4 * U * ref.abs() + 1e-7   # logf on an exact argument
    check(f'log_det_exact/{"x".join(map(str, dims))}', 'log det (in units of the bound)', (ld[pos].double() - ref) / tol,
          torch.zeros_like(ref), 1.0)
    want = [int(neg[c].sum()) for c in range(C)]
    assert len(set(want)) == C, want   # the chains fold differently: a counter that is not per chain cannot pass
    assert cnt.cpu().tolist() == want
    # without the map: the counts alone
    lib_cnt = torch.empty(C, device=DEV, dtype=torch.int64)
    from ir_sgmcmc_amd import _lib as L
    L.check(L.load().irs_log_det_jacobian(L.dev_ptr(t_d, torch.float32), None, L.dev_ptr(lib_cnt), C, *dims, L.stream_ptr()))
    assert lib_cnt.cpu().tolist() == want


@pytest.mark.parametrize('dims', X.EXACT_DIMS)
def test_jacobian_posterior_sees_the_same_folds(dims):
    """irs_jacobian_posterior_update shares det_jacobian with the fold count: a record is a fold where det J is not > 0"""
    t, _, det = _exact(dims)
    C = t.shape[0]
    state = lambda: (torch.zeros(dims, device=DEV, dtype=torch.int32), torch.zeros(dims, device=DEV), torch.zeros(dims, device=DEV))
    for c in range(C):
        folds, mean, m2 = state()
        G.jacobian_posterior_update(dev(t[c:c + 1]), folds, mean, m2, 0)
        assert torch.equal(folds.cpu() == 1, det[c] <= 0), c
        assert int(folds.max()) <= 1
    folds, mean, m2 = state()
    G.jacobian_posterior_update(dev(t), folds, mean, m2, 0)
    assert torch.equal(folds.cpu().long(), (det <= 0).sum(0))


# ---------------------------------------------------------------- log det J, smooth folding fields
@pytest.mark.parametrize('dims,amp', [((10, 14, 22), 6.0), ((7, 70, 13), 30.0)])
def test_log_det_jacobian_on_smooth_folding_fields(dims, amp):
    """With S the sum of the absolute six triple products (fp64), det computed in fp32 is within B = 16 * 2^-24 * S of the fp64
    one: nine entries of 2.5 roundings each, products of three factors, five additions.  Where B <= |det| / 2 the sign is
    decided: NaN-ness equals det < 0 and |ld - log det| <= 2 B / |det| + 4 * 2^-24 |log det| + 1e-7.  The other voxels (at most
    1e-3 of them; 0 and 7.8e-5 with the fp32 oracle in place of the kernel) are left out, and the counts may differ by them."""
    t, _ = O.svf_exp(smooth_field(2, dims, amp, 9))
    t = t.contiguous()
    C = t.shape[0]
    nabla = O.forward_differences(t.double(), transformation=True)
    a, b, c = nabla[..., 0], nabla[..., 1], nabla[..., 2]
    prods = [a[:, 0] * b[:, 1] * c[:, 2], b[:, 0] * c[:, 1] * a[:, 2], c[:, 0] * a[:, 1] * b[:, 2],
             a[:, 2] * b[:, 1] * c[:, 0], b[:, 2] * c[:, 1] * a[:, 0], c[:, 2] * a[:, 1] * b[:, 0]]
    det = O.det_jacobian(nabla)
    assert torch.equal(det, prods[0] + prods[1] + prods[2] - prods[3] - prods[4] - prods[5])
    B = 16 * U * sum(p.abs() for p in prods)
    decided = B <= 0.5 * det.abs()
    left_out = (~decided).reshape(C, -1).sum(1)
    assert float((~decided).double().mean()) <= 1e-3
    assert int((det < 0).sum()) > 0   # the field folds

    cnt, ld = G.log_det_jacobian(dev(t))
    ld = ld.cpu()
    T = f'log_det_smooth/{"x".join(map(str, dims))}_amp{amp:g}'
    assert torch.equal(torch.isnan(ld)[decided], (det < 0)[decided])
    ok = decided & (det > 0)
    ref = det[ok].log()
    tol = 2 * B[ok] / det[ok].abs() + 4 * U * ref.abs() + 1e-7
    check(T, 'log det (in units of the bound)', (ld[ok].double() - ref) / tol, torch.zeros_like(ref), 1.0)
    for ch in range(C):
        assert abs(int(cnt[ch]) - int((det[ch] < 0).sum())) <= int(left_out[ch]), ch
        assert int(cnt[ch]) == int(torch.isnan(ld[ch]).sum())
