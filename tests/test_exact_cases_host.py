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


# ---------------------------------------------------------------- squaring steps
def _step_grid(case):
    return X.identity(case.dims, torch.float64) + case.D.double()


@pytest.mark.parametrize('dims', X.EXACT_DIMS)
def test_step_case_is_exact_in_fp32(dims):
    """one step and its adjoint: fp32 == fp64 bit for bit through ATen and through the explicit restatement, which agree in fp64"""
    case = X.step_case(dims)
    assert case.D.shape == case.G.shape == (5, 3, *dims) and case.D.dtype == torch.float32
    assert torch.equal(case.G, case.G.round()) and float(case.G.abs().max()) == 8.0
    quarter = X.O.to_voxels(case.D.double()) * 4.0
    assert torch.equal(quarter, quarter.round())
    out64, gd64 = X.step_reference(case.D, case.G, torch.float64)
    for explicit in (False, True):
        out32, gd32 = X.step_reference(case.D, case.G, torch.float32, explicit)
        assert same_bits(out32, out64), ('step', explicit)
        assert same_bits(gd32, gd64), ('adjoint', explicit)
    oute, gde = X.step_reference(case.D, case.G, torch.float64, explicit=True)
    assert torch.equal(oute, out64) and torch.equal(gde, gd64)
    # what the stateless adjoint returns for this case (tests/test_gpu_exp_exact.py, b and c): the adjoint over n_c - 1, a power of two
    gv64 = X.chain_reference(2.0 * X.O.to_voxels(case.D), 1, torch.float64, case.G)[3]
    gv32 = X.chain_reference(2.0 * X.O.to_voxels(case.D), 1, torch.float32, case.G)[3]
    scale = torch.tensor([1.0 / (n - 1) for n in X.axis_sizes(dims)], dtype=torch.float64).view(1, 3, 1, 1, 1)
    assert same_bits(gv32, gv64) and torch.equal(gv64, gd64 * scale)
    for c in range(5):   # every chain's gradient differs from its upstream gradient and from the other chains'
        assert not torch.equal(gd64[c], case.G[c].double())


@pytest.mark.parametrize('dims', X.EXACT_DIMS)
def test_step_case_holds_its_amplitude_classes_and_the_hard_positions(dims):
    """floor(max|d|) + 1 = 1, 2, 2, 3 and more than 3: the radius-1 gather, the radius-2 gather twice (at exactly one voxel and
    below two), the any-radius kernel twice (at exactly two voxels and far beyond).  The four class shares are asked of every
    case, (2, 3, 5) included, pooled over the five chains and the three axes.  Asked per axis as well: the extremes, and the
    share of interior voxel centres -- from which the z axis of (2, 3, 5) is exempt, n = 2 has no interior centre.  Asked per
    chain as well: a coordinate on each border, below and above the volume -- from which (2, 3, 5) is exempt, 30 voxels a chain
    do not hold all four on every axis whatever the draw; there the five chains are taken together."""
    case = X.step_case(dims)
    widths = X.step_widths(case.D)
    assert tuple(widths[:4]) == X.STEP_WIDTHS and widths[4] > 3, widths
    vox = X.O.to_voxels(case.D.double())
    for chain, a in enumerate(X.STEP_REACH):
        assert float(vox[chain].abs().max()) == a / 4.0
        for (z, y, x), sign in X.extreme_voxels(dims):
            assert vox[chain, :, z, y, x].tolist() == [sign * a / 4.0] * 3
    D, H, W = dims
    (far, _), (_, _), (face, _), (row, _) = X.extreme_voxels(dims)
    assert far[2] // 32 == (W - 1) // 32 and (W % 32 == 1 or W < 32) and far[1] // 8 == (H - 1) // 8 and (H % 8 == 1 or H < 8)   # ragged last tile
    assert face[2] == 0 and row[1] == H - 1
    grid = _step_grid(case)
    share = X.coordinate_classes(grid, dims)
    for k in ('border', 'below', 'above', 'centre'):
        assert share[k] >= MIN_SHARE, (k, share)
    for c, (raw, n) in enumerate(zip(X.voxel_coordinates(grid, dims), X.axis_sizes(dims))):
        assert float(raw.min()) == -3.0 and float(raw.max()) == n - 1 + 3.0
        # every chain: coordinates exactly on both borders, below and above the volume ((2, 3, 5) has 30 voxels: the five together)
        for r in (raw if raw[0].numel() > 1000 else [raw]):
            assert int((r == 0).sum()) > 0 and int((r == n - 1).sum()) > 0 and int((r < 0).sum()) > 0 and int((r > n - 1).sum()) > 0, c
        if n > 2:
            inside = (raw > 0) & (raw < n - 1)
            assert int((inside & (raw == raw.floor())).sum()) >= MIN_SHARE * raw.numel(), c
    assert len({case.D[c].abs().sum().item() for c in range(5)}) == 5


@pytest.mark.parametrize('dims', X.EXACT_DIMS)
def test_the_adjoint_of_a_step_at_zero_doubles_its_input(dims):
    """d = 0: the sample is the field itself and its coordinate gradient vanishes, so the adjoint is G + G (what makes step 0 of the
    injected two-step call of tests/test_gpu_exp_exact.py an exact factor)"""
    case = X.step_case(dims)
    zero = torch.zeros_like(case.D)
    for dtype in (torch.float32, torch.float64):
        for explicit in (False, True):
            out, gd = X.step_reference(zero, case.G, dtype, explicit)
            assert torch.equal(gd, 2.0 * case.G.to(dtype)) and torch.equal(out, zero.to(dtype))


@pytest.mark.parametrize('dims', X.EXACT_DIMS)
def test_a_restatement_with_another_border_rule_is_noticed(dims, monkeypatch):
    """the coordinate gradient left ON at i = 0 and i = n - 1 (`<=` for `<`): the cases hold enough coordinates exactly on a border,
    next to values that differ, for the adjoint to come out different in every chain"""
    case = X.step_case(dims)
    _, right = X.step_reference(case.D, case.G, torch.float64, explicit=True)

    def closed(g, size):
        i = ((g + 1.0) / 2.0) * (size - 1)
        return i.clamp(0, size - 1), ((i >= 0) & (i <= size - 1)).to(g.dtype) * ((size - 1) / 2.0)
    monkeypatch.setattr(X.O, '_unnormalise_clip', closed)
    out, wrong = X.step_reference(case.D, case.G, torch.float64, explicit=True)
    assert torch.equal(out, X.step_reference(case.D, case.G, torch.float64)[0])   # the forward step does not see the rule
    for chain in range(5):
        assert not torch.equal(wrong[chain], right[chain]), chain
    # ... and only where a coordinate is exactly on a border
    raw = X.voxel_coordinates(_step_grid(case), dims)
    on_border = torch.stack([(r == 0) | (r == n - 1) for r, n in zip(raw, X.axis_sizes(dims))], 1)
    assert int(((wrong != right) & ~on_border).sum()) == 0 and int((wrong != right).sum()) > 0


VELOCITY = [(dims, name) for dims in X.EXACT_DIMS for name in X.VELOCITY_CASES]


@pytest.mark.parametrize('dims,name', VELOCITY)
def test_velocity_case_is_exact_in_fp32(dims, name):
    """every field of the chain, the transformation and the displacement: fp32 == fp64 bit for bit; one step: grad_v too (of two
    steps it is not exact, DESIGN.md "Numerics note (exact cases)", and is not asked for)"""
    case = X.velocity_case(dims, name)
    n = case.no_steps
    lattice = case.v.double() / 2 ** n * (4 if n == 1 else 2)
    assert torch.equal(lattice, lattice.round()) and case.v.shape == (case.C, 3, *dims)
    g_last = X.step_case(dims).G[:case.C] if n == 1 else None
    t32, u32, s32, gv32 = X.chain_reference(case.v, n, torch.float32, g_last)
    t64, u64, s64, gv64 = X.chain_reference(case.v, n, torch.float64, g_last)
    assert len(s64) == n + 1 and same_bits(t32, t64) and same_bits(u32, u64)
    for a, b in zip(s32, s64):
        assert same_bits(a, b)
    assert torch.equal(X.O.to_voxels(s64[0]), case.v.double() / 2 ** n)
    if n == 1:
        assert same_bits(gv32, gv64)
    # the restated step gives the same chain
    d = s64[0]
    for k in range(n):
        d, _ = X.step_reference(d, torch.zeros_like(d), torch.float64, explicit=True)
        assert torch.equal(d, s64[k + 1]), k
    for a in range(case.C):
        for b in range(a + 1, case.C):
            assert not torch.equal(case.v[a], case.v[b])


def _below_one(w):
    return w == 1


def _one_to_two(w):
    return w == 2


def _two_or_more(w):
    return w >= 3


# floor(max|d_k|) + 1 per chain, for k = 0 .. no_steps - 1 (the fields a step READS): what each case was built to select
VELOCITY_WIDTHS = {
    'one step': [[_below_one, _below_one, _one_to_two, _two_or_more]],
    'two steps': [[_below_one, _below_one, _one_to_two, _two_or_more], [_below_one, _one_to_two, _two_or_more, _two_or_more]],
    'two steps, far': [[_below_one, _two_or_more], [_one_to_two, _two_or_more]],
    'engine': [[_below_one, _below_one, _two_or_more], [_below_one, _one_to_two, _two_or_more]],
}


@pytest.mark.parametrize('dims,name', VELOCITY)
def test_velocity_case_puts_its_chains_on_both_sides_of_one_and_two_voxels(dims, name):
    case = X.velocity_case(dims, name)
    _, _, steps, _ = X.chain_reference(case.v, case.no_steps, torch.float64)
    for k, classes in enumerate(VELOCITY_WIDTHS[name]):
        widths = X.step_widths(steps[k])
        assert all(ok(w) for ok, w in zip(classes, widths)), (k, widths)
    if name == 'two steps, far' and min(dims) > 5:
        assert X.step_widths(steps[2])[1] > 12, X.step_widths(steps[2])   # the last field reaches far out of any ring


@pytest.mark.parametrize('n', [2, 3, 5, 6, 128, 130, 132])
def test_the_identity_table_is_one_rounding_from_linspace(n):
    """fp32 linspace(-1, 1, n) as torch's CPU kernel evaluates it (csrc/field_kernels.hip: fill_linspace repeats it) against the
    float64 one: a rounded step, a rounded product and a rounded sum, yet within 2^-24 -- the rounding of one fp32 operation on
    values up to 2 -- at the sizes of test_outputs_kernel_rounds_once_per_operation, whose bound starts from that"""
    err = (torch.linspace(-1, 1, n).double() - torch.linspace(-1, 1, n, dtype=torch.float64)).abs()
    assert float(err.max()) <= 2.0 ** -24


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
