"""The exact ("dyadic") cases of tests/_exact_cases.py, host side: on every case the GPU tests use, the fp32 oracle equals the
fp64 oracle bit for bit (so the kernels may be held to torch.equal), every case holds the hard positions it was built for, the
integer restatement of the Philox jitter gives the Random123 known answers, and the warp / LCC wrappers refuse wrong shapes."""
import numpy as np
import pytest
import torch

from ir_sgmcmc_amd import _lib as L
from ir_sgmcmc_amd import ops as G
from tests import _exact_cases as X

MIN_SHARE = 0.01   # every class of position: at least 1 % of the coordinates of a case


def same_bits(a32, a64):
    return a32.dtype == torch.float32 and a64.dtype == torch.float64 and torch.equal(a32.double(), a64)


# ---------------------------------------------------------------- trilinear warp
@pytest.mark.parametrize('jitter', [False, True])
@pytest.mark.parametrize('dims,per_chain', X.WARP_CASES)
def test_warp_case_is_exact_in_fp32(dims, per_chain, jitter):
    case = X.warp_case(dims, per_chain)
    assert case.im.shape == ((X.CHAINS if per_chain else 1), 1, *dims) and case.d_last.shape == (X.CHAINS, 3, *dims)
    for t in (case.im, case.g_warped, case.unif * 8):
        assert torch.equal(t, t.round())
    assert float(case.unif.min()) >= 0.0 and float(case.unif.max()) < 1.0
    out64, gd64, grid64 = X.warp_reference(case, torch.float64, jitter)
    for explicit in (False, True):
        out32, gd32, grid32 = X.warp_reference(case, torch.float32, jitter, explicit)
        assert same_bits(grid32, grid64)
        assert same_bits(out32, out64), ('value', explicit)
        assert same_bits(gd32, gd64), ('grid gradient', explicit)
    oute, gde, _ = X.warp_reference(case, torch.float64, jitter, explicit=True)
    assert torch.equal(oute, out64) and torch.equal(gde, gd64)
    assert float(gd64.abs().max()) > 0 and float(out64.std()) > 0


@pytest.mark.parametrize('jitter', [False, True])
@pytest.mark.parametrize('dims,per_chain', X.WARP_CASES)
def test_warp_case_holds_the_hard_positions(dims, per_chain, jitter):
    case = X.warp_case(dims, per_chain)
    grid, _ = X.warp_grid(case, torch.float64, jitter)
    share = X.coordinate_classes(grid.detach(), dims)
    for k in ('border', 'below', 'above', 'centre'):
        assert share[k] >= MIN_SHARE, (k, share)
    if not jitter:   # the displacement reaches `reach` = 3 voxels past every face of every axis
        for raw, n in zip(X.voxel_coordinates(grid.detach(), dims), X.axis_sizes(dims)):
            assert float(raw.min()) == -3.0 and float(raw.max()) == n - 1 + 3.0
            assert int((raw == 0).sum()) > 0 and int((raw == n - 1).sum()) > 0
    # chains differ (a kernel that reads chain 0's field for every chain must not pass)
    assert not torch.equal(case.d_last[0], case.d_last[1]) and not torch.equal(case.d_last[0], case.d_last[2])
    if per_chain:
        assert not torch.equal(case.im[0], case.im[1]) and not torch.equal(case.im[0], case.im[2])


def test_a_builder_without_hard_positions_is_noticed():
    """the class shares do tell a lattice that avoids the hard positions from one that holds them"""
    dims = (9, 17, 33)
    ident = X.identity(dims, torch.float64).repeat(2, 1, 1, 1, 1)
    share = X.coordinate_classes(ident, dims)   # the identity: centres and borders only
    assert share['below'] == 0 and share['above'] == 0 and share['tie_even'] == 0 and share['border'] > 0
    assert abs(share['border'] + share['centre'] - 1.0) < 1e-12
    off = ident + 0.3 * 2.0 / 32   # 0.3 voxels off in every axis (in units of the longest): no coordinate on a centre or a border
    share = X.coordinate_classes(off, dims)
    assert share['centre'] == 0 and share['border'] == 0


# ---------------------------------------------------------------- nearest warp
@pytest.mark.parametrize('dims', X.EXACT_DIMS)
def test_nearest_case_is_exact_and_full_of_ties(dims):
    case = X.nearest_case(dims)
    t = case.transformation
    assert case.labels_shared.dtype == torch.int16 and case.mask_chain.dtype == torch.bool
    assert case.labels_shared.shape == (1, 1, *dims) and case.labels_chain.shape == (X.CHAINS, 1, *dims)
    for seg in (case.labels_shared, case.labels_chain, case.mask_shared, case.mask_chain):
        assert torch.equal(X.nearest_reference(seg, t, torch.float32), X.nearest_reference(seg, t, torch.float64))
    share = X.coordinate_classes(t, dims)
    for k in ('border', 'below', 'above', 'centre', 'tie_even', 'tie_odd'):
        assert share[k] >= MIN_SHARE, (k, share)
    # the ties matter: rounding half away from zero picks another voxel than rounding half to even at the even-floor ties
    # (0.5 -> 0, 2.5 -> 2), and the label images differ between neighbours almost everywhere
    raw = X.voxel_coordinates(t, dims)
    clipped = [r.clamp(0, n - 1) for r, n in zip(raw, X.axis_sizes(dims))]
    even = [torch.from_numpy(np.rint(c.numpy())) for c in clipped]
    away = [torch.floor(c + 0.5) for c in clipped]
    assert sum(int((e != a).sum()) for e, a in zip(even, away)) >= MIN_SHARE * 3 * raw[0].numel()
    assert len(torch.unique(case.labels_chain)) > 100 or case.labels_chain.numel() < 200


# ---------------------------------------------------------------- Jacobian
@pytest.mark.parametrize('dims', X.EXACT_DIMS)
def test_transformation_case_is_exact_and_folds_differently_per_chain(dims):
    t = X.transformation_case(dims)
    assert t.shape == (X.CHAINS, 3, *dims) and t.dtype == torch.float32
    nab32, det32 = X.jacobian_reference(t, torch.float32)
    nab64, det64 = X.jacobian_reference(t, torch.float64)
    assert same_bits(nab32, nab64) and same_bits(det32, det64)
    folds = [int((det64[c] < 0).sum()) for c in range(X.CHAINS)]
    assert len(set(folds)) == X.CHAINS and min(folds) > 0, folds
    assert int((det64 > 0).sum()) > 0
    if t[0, 0].numel() > 1000:
        assert int((det64 == 0).sum()) >= 10   # det J == 0: log gives -inf, which is no fold


# ---------------------------------------------------------------- Philox restatement
@pytest.mark.parametrize('ctr,key,expect', [((0, 0), 0, (0xff1dae59, 0x6cd10df2)),
                                            ((0xffffffff, 0xffffffff), 0xffffffff, (0x2c3f628b, 0xab4fd7ad)),
                                            ((0x243f6a88, 0x85a308d3), 0x13198a2e, (0xdd7ce038, 0xf62a4c12))])
def test_philox2x32_10_known_answers(ctr, key, expect):
    """Random123's kat_vectors for philox2x32 with 10 rounds"""
    x, y = X.philox2x32_10(ctr[0], ctr[1], key)
    assert (int(x), int(y)) == expect
    xs, ys = X.philox2x32_10(np.full(5, ctr[0], dtype=np.uint64), np.full(5, ctr[1], dtype=np.uint64), key)   # vectorised alike
    assert xs.tolist() == [expect[0]] * 5 and ys.tolist() == [expect[1]] * 5


def test_philox_jitter_uniforms_layout():
    dims, C = (3, 4, 5), 3
    V = 60
    u = X.philox_jitter_uniforms(5, 7, C, dims)
    assert u.shape == (C, 3, *dims) and u.dtype == torch.float32
    r = u.double() * 2097152.0
    assert torch.equal(r, r.round()) and float(u.min()) >= 0.0 and float(u.max()) < 1.0
    # one voxel by hand: chain 2, voxel 17 -> counter (2 V + 17, 7 << 4), key_mix(5, 7, 0x554E)
    x, y = (int(w) for w in X.philox2x32_10(2 * V + 17, 7 << 4, X.key_mix(5, 7, 0x554E)))
    want = [(x >> 11) / 2 ** 21, (y >> 11) / 2 ** 21, ((x & 0x7FF) | ((y & 0x3FF) << 11)) / 2 ** 21]
    assert u.reshape(C, 3, V)[2, :, 17].tolist() == want
    # chain c of a C-chain call is the whole-volume index c * Vg on: a slab of a larger volume draws what the volume would
    big = X.philox_jitter_uniforms(5, 7, 1, (2 * V + 60,))
    assert torch.equal(u.reshape(C, 3, V)[2], big[0, :, 2 * V:3 * V])
    assert torch.equal(X.philox_jitter_uniforms(5, 7, 2, dims, Vg=2 * V)[1], u[2])
    # the iteration enters the counter with its low 28 bits and the key with the rest; the seed enters the key
    assert X.key_mix(5, 3, 0x554E) == X.key_mix(5, 2 ** 28 - 1, 0x554E) != X.key_mix(5, 2 ** 28 + 3, 0x554E)
    assert X.key_mix(5, 3, 0x554E) != X.key_mix(6, 3, 0x554E)
    a, b, c = (X.philox_jitter_uniforms(5, it, 1, dims) for it in (3, 2 ** 28 + 3, 4))
    assert not torch.equal(a, b) and not torch.equal(a, c)
    # an index above 2^32 moves into the second counter word (next to the iteration's bits)
    hi = X.philox_jitter_uniforms(5, 3, 2, (1, 1, 2), Vg=2 ** 32 + 1)[1].reshape(3, 2)[:, 0]
    x, y = (int(w) for w in X.philox2x32_10(1, 1 | (3 << 4), X.key_mix(5, 3, 0x554E)))
    assert hi[0].item() == (x >> 11) / 2 ** 21 and hi[1].item() == (y >> 11) / 2 ** 21


def test_philox_jitter_uniforms_statistics():
    u = X.philox_jitter_uniforms(1, 2, 3, (16, 16, 16)).double()
    n = u[0, 0].numel() * 3
    for c in range(3):
        x = u[:, c].flatten()
        assert abs(float(x.mean()) - 0.5) < 5.0 * (1.0 / 12.0 / n) ** 0.5
        assert abs(float(((x - 0.5) ** 2).mean()) - 1.0 / 12.0) < 5.0 * (1.0 / 180.0 / n) ** 0.5
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert abs(float(((u[:, a] - 0.5) * (u[:, b] - 0.5)).mean()) * 12.0) < 5.0 / n ** 0.5


# ---------------------------------------------------------------- shape checks of the wrappers (no kernel runs: they raise first)
def _shapes(C=2, dims=(6, 7, 8)):
    z = lambda *s: torch.zeros(*s)
    return C, dims, z


@pytest.mark.parametrize('bad', [(1, 1, 6, 7, 9), (1, 1, 7, 6, 8), (3, 1, 6, 7, 8), (2, 2, 6, 7, 8), (1, 6, 7, 8), (2, 1, 5, 7, 8)])
def test_warp_displacement_refuses_an_image_of_another_shape(bad):
    C, dims, z = _shapes()
    d = z(C, 3, *dims)
    with pytest.raises(L.IrsError, match='image shape .* does not match d_last'):
        G.warp_displacement(z(*bad), d)
    with pytest.raises(L.IrsError, match='image shape .* does not match d_last'):
        G.warp_displacement_bwd(z(*bad), d, z(C, 1, *dims))


def test_warp_displacement_refuses_other_operands_of_another_shape():
    C, dims, z = _shapes()
    d, im = z(C, 3, *dims), z(1, 1, *dims)
    for unif in (z(1, 3, *dims), z(C, 1, *dims), z(C, 3, 6, 7, 9)):
        with pytest.raises(L.IrsError, match='unif shape .* does not match d_last'):
            G.warp_displacement(im, d, unif, 0.1)
        with pytest.raises(L.IrsError, match='unif shape .* does not match d_last'):
            G.warp_displacement_bwd(im, d, z(C, 1, *dims), unif, 0.1)
    for gw in (z(1, 1, *dims), z(C, 3, *dims), z(C, *dims), z(C, 1, 6, 7, 9)):
        with pytest.raises(L.IrsError, match='g_warped shape .* does not match d_last'):
            G.warp_displacement_bwd(im, d, gw)
    with pytest.raises(L.IrsError):
        G.warp_displacement(im, z(C, 2, *dims))


@pytest.mark.parametrize('bad', [(1, 1, 6, 7, 9), (3, 1, 6, 7, 8), (2, 2, 6, 7, 8), (1, 6, 7, 8), (2, 1, 8, 7, 6)])
def test_lcc_map_refuses_a_fixed_image_of_another_shape(bad):
    C, dims, z = _shapes()
    w = z(C, 1, *dims)
    with pytest.raises(L.IrsError, match='fhat shape .* does not match warped'):
        G.lcc_map_fwd(z(*bad), w, 1)
    with pytest.raises(L.IrsError, match='fhat shape .* does not match z'):
        G.lcc_map_bwd(z(*bad), w, w, w, 1)


def test_lcc_map_bwd_refuses_other_operands_of_another_shape():
    C, dims, z = _shapes()
    w, fhat = z(C, 1, *dims), z(1, 1, *dims)
    for bad in (z(1, 1, *dims), z(C, 1, 6, 7, 9), z(C, *dims)):
        with pytest.raises(L.IrsError, match='sigma_m shape .* does not match z'):
            G.lcc_map_bwd(fhat, w, bad, w, 1)
        with pytest.raises(L.IrsError, match='g_z shape .* does not match z'):
            G.lcc_map_bwd(fhat, w, w, bad, 1)


def test_wrappers_reach_the_device_check_with_matching_shapes():
    """matching shapes pass the shape checks: what stops a host tensor is the device check behind them"""
    C, dims, z = _shapes()
    with pytest.raises(L.IrsError, match='GPU only'):
        G.warp_displacement(z(C, 1, *dims), z(C, 3, *dims), z(C, 3, *dims), 0.1)
    with pytest.raises(L.IrsError, match='GPU only'):
        G.lcc_map_bwd(z(C, 1, *dims), z(C, 1, *dims), z(C, 1, *dims), z(C, 1, *dims), 1)
