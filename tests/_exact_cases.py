"""Exact ("dyadic") inputs for the warp family and the Jacobian operators, shared by the host and GPU tests (DESIGN.md,
"Numerics": the exact-case method), and an integer restatement of the Philox jitter of the warp.

When every dimension is 2^k + 1, the linspace(-1, 1, n) tables, 2 / (n - 1) and ((g + 1) * 0.5) * (n - 1) are exact in fp32.
Displacements on a 1/4-voxel lattice (1/8 with the dyadic jitter draws) then give exactly representable interpolation weights,
and with small-integer image values every product and every sum of the sampler, of its adjoint and of det J is exact: fp32
and fp64 agree bit for bit (tests/test_exact_cases_host.py proves that for every case the GPU tests use), so a kernel may be
held to torch.equal.  Any difference is an indexing, clamp, weight or stride error; there is no rounding to hide behind.

The builders are seeded and return CPU tensors.
"""
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from oracle import ops as O

# (5, 9, 129): three x-blocks of 64 lanes, and H = 9 leaves the second 8-row block of the forward warp one real row and its
# clamped repeat; (33, 5, 65): H smaller than the 8 rows of one block; (2, 3, 5): the smallest volume the ABI admits
EXACT_DIMS = [(9, 17, 33), (5, 9, 129), (33, 5, 65), (2, 3, 5)]
CHAINS = 3
ALPHA = 0.5   # jitter magnitude of the exact cases: -2 alpha u + alpha is a multiple of 1/8 voxel for u on the 1/8 lattice


def axis_sizes(dims):
    """channel c of a field (x, y, z) <-> (W, H, D)"""
    return dims[2], dims[1], dims[0]


def identity(dims, dtype=torch.float32):
    """(1,3,D,H,W) identity transformation in [-1,1] (exact in fp32 for dyadic dims)"""
    return O.identity_grid(dims).permute(0, 4, 1, 2, 3).contiguous().to(dtype)


def _index_grids(dims):
    z, y, x = torch.meshgrid(*(torch.arange(n) for n in dims), indexing='ij')
    return x, y, z


def _positions(n, shape, step, reach, g):
    """Sampling positions in voxels on the 1/step lattice: 60 % uniform over [-reach, n - 1 + reach], 15 % exactly on one of
    the two borders, 25 % exactly on an interior voxel centre (n = 2 has none: those land on the border)."""
    uni = torch.randint(-reach * step, (n - 1 + reach) * step + 1, shape, generator=g)
    border = torch.randint(0, 2, shape, generator=g) * ((n - 1) * step)
    centre = torch.randint(1, max(n - 1, 2), shape, generator=g) * step
    pick = torch.rand(shape, generator=g)
    pos = torch.where(pick < 0.6, uni, torch.where(pick < 0.75, border, centre))
    # the two extremes and the two borders are there whatever the draw (a tiny volume has few coordinates)
    where = torch.randperm(pos.numel(), generator=g)[:4]
    pos.view(-1)[where] = torch.tensor([-reach * step, (n - 1 + reach) * step, 0, (n - 1) * step])
    return pos.double() / step


def dyadic_warp_case(dims, C=CHAINS, per_chain=False, frac=4, reach=3, seed=0):
    """Inputs of the trilinear warp and its adjoint on which fp32 arithmetic is exact.
    im (C or 1, 1, *dims): integers 0..255; d_last (C,3,*dims) = q * 2 / (n - 1) per axis with id + q on the 1/frac-voxel
    lattice, reaching `reach` (>= 3) voxels past every face; g_warped (C,1,*dims): integers -8..8; unif (C,3,*dims): multiples
    of 1/8 in [0,1) for the injected jitter at alpha = ALPHA."""
    assert reach >= 3 and all(((n - 1) & (n - 2)) == 0 for n in dims), 'every dim must be 2^k + 1'
    g = torch.Generator().manual_seed(seed)
    im = torch.randint(0, 256, (C if per_chain else 1, 1, *dims), generator=g).float()
    d = torch.empty(C, 3, *dims, dtype=torch.float64)
    for c, (n, idx) in enumerate(zip(axis_sizes(dims), _index_grids(dims))):
        d[:, c] = (_positions(n, (C, *dims), frac, reach, g) - idx) * (2.0 / (n - 1))
    g_warped = torch.randint(-8, 9, (C, 1, *dims), generator=g).float()
    unif = torch.randint(0, 8, (C, 3, *dims), generator=g).float() / 8.0
    assert torch.equal(d.float().double(), d)
    return SimpleNamespace(dims=tuple(dims), C=C, per_chain=per_chain, im=im, d_last=d.float().contiguous(), g_warped=g_warped,
                           unif=unif, alpha=ALPHA)


def dyadic_nearest_case(dims, C=CHAINS, reach=3, seed=0):
    """Label images (int16 and bool, shared and per chain) and a transformation (C,3,*dims) whose positions lie on the
    half-voxel lattice: about half of the coordinates inside the volume are exact ties of the rounding."""
    assert all(((n - 1) & (n - 2)) == 0 for n in dims), 'every dim must be 2^k + 1'
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(-300, 3000, (C, 1, *dims), generator=g).to(torch.int16)
    msk = torch.rand(C, 1, *dims, generator=g) > 0.5
    t = torch.empty(C, 3, *dims, dtype=torch.float64)
    for c, n in enumerate(axis_sizes(dims)):
        t[:, c] = -1.0 + _positions(n, (C, *dims), 2, reach, g) * (2.0 / (n - 1))
    assert torch.equal(t.float().double(), t)
    return SimpleNamespace(dims=tuple(dims), C=C, labels_shared=lab[:1].contiguous(), labels_chain=lab, mask_shared=msk[:1].contiguous(),
                           mask_chain=msk, transformation=t.float().contiguous())


def dyadic_transformation(dims, C=CHAINS, seed=0):
    """identity + a white displacement on the quarter-voxel lattice, (C,3,*dims); chain c has amplitude (2 + 5 c) / 4 voxels,
    so the chains fold at different rates.  Every entry of the Jacobian is a multiple of 1/4 times a ratio of two (n - 1), a power
    of two, and det J is exact in fp32."""
    assert all(((n - 1) & (n - 2)) == 0 for n in dims), 'every dim must be 2^k + 1'
    g = torch.Generator().manual_seed(seed)
    t = identity(dims, torch.float64).repeat(C, 1, 1, 1, 1)
    for chain in range(C):
        a = 2 + 5 * chain
        for c, n in enumerate(axis_sizes(dims)):
            t[chain, c] += torch.randint(-a, a + 1, dims, generator=g).double() / 4.0 * (2.0 / (n - 1))
    assert torch.equal(t.float().double(), t)
    return t.float().contiguous()


# ---- the cases the GPU tests run; tests/test_exact_cases_host.py proves fp32 == fp64 on each of them
WARP_CASES = [(dims, per_chain) for dims in EXACT_DIMS for per_chain in (False, True)]


def warp_case(dims, per_chain):
    return dyadic_warp_case(dims, CHAINS, per_chain, frac=4, reach=3, seed=1000 + 2 * EXACT_DIMS.index(tuple(dims)) + int(per_chain))


def nearest_case(dims):
    return dyadic_nearest_case(dims, CHAINS, reach=3, seed=2000 + EXACT_DIMS.index(tuple(dims)))


def transformation_case(dims):
    return dyadic_transformation(dims, CHAINS, seed=3000 + EXACT_DIMS.index(tuple(dims)))


# ---- references (dtype = torch.float32 or torch.float64)
def warp_grid(case, dtype, jitter):
    """the sampling grid (C,3,*dims) of a warp case as a function of d_last: (grid, d_last leaf)"""
    d = case.d_last.to(dtype).clone().requires_grad_(True)
    grid = identity(case.dims, dtype) + d
    if jitter:
        grid = O.jitter_grid(grid, case.alpha, case.unif.to(dtype))
    return grid, d


def warp_reference(case, dtype, jitter=False, explicit=False):
    """-> (warped (C,1,*dims), d(sum(warped * g_warped)) / d(d_last) (C,3,*dims), grid (C,3,*dims)), all in `dtype`;
    explicit: the oracle's own restatement of the sampler and its adjoint instead of ATen's grid_sample + autograd"""
    grid, d = warp_grid(case, dtype, jitter)
    im = case.im.to(dtype).expand(case.C, -1, -1, -1, -1)
    gw = case.g_warped.to(dtype)
    if explicit:
        g5 = grid.detach().permute(0, 2, 3, 4, 1)
        out = O.trilinear_sample_explicit(im, g5)
        _, gg = O.trilinear_backward_explicit(im, g5, gw, need_input_grad=False)
        return out, gg.permute(0, 4, 1, 2, 3).contiguous(), grid.detach()
    out = O.warp_trilinear(im, grid)
    gd, = torch.autograd.grad(out, d, gw)
    return out.detach(), gd, grid.detach()


def nearest_reference(seg, transformation, dtype):
    """F.grid_sample(mode='nearest') of a label image (1 or C chains) evaluated in `dtype`, cast back"""
    C = transformation.shape[0]
    out = F.grid_sample(seg.to(dtype).expand(C, -1, -1, -1, -1), transformation.to(dtype).permute(0, 2, 3, 4, 1), mode='nearest',
                        padding_mode='border', align_corners=True)
    return out.to(seg.dtype)


def jacobian_reference(transformation, dtype):
    """-> (forward_differences(t, True) (C,3,D,H,W,3), det J (C,D,H,W)) in `dtype`"""
    nabla = O.forward_differences(transformation.to(dtype), transformation=True)
    return nabla, O.det_jacobian(nabla)


def voxel_coordinates(grid, dims):
    """unnormalised, unclipped coordinates ((g + 1) / 2) * (n - 1) of a grid (C,3,*dims), in float64: a list per axis"""
    return [((grid[:, c].double() + 1.0) / 2.0) * (n - 1) for c, n in enumerate(axis_sizes(dims))]


def coordinate_classes(grid, dims):
    """Share of the coordinates (the three axes pooled) in each class of position the clamp logic of the samplers tells apart;
    the tie classes are those of round-half-to-even inside the volume."""
    cnt = dict(border=0, below=0, above=0, centre=0, tie_even=0, tie_odd=0)
    total = 0
    for raw, n in zip(voxel_coordinates(grid, dims), axis_sizes(dims)):
        inside = (raw > 0) & (raw < n - 1)
        fl = raw.floor()
        tie = inside & (raw - fl == 0.5)
        cnt['border'] += int(((raw == 0) | (raw == n - 1)).sum())
        cnt['below'] += int((raw < 0).sum())
        cnt['above'] += int((raw > n - 1).sum())
        cnt['centre'] += int((inside & (raw == fl)).sum())
        cnt['tie_even'] += int((tie & (fl % 2 == 0)).sum())
        cnt['tie_odd'] += int((tie & (fl % 2 == 1)).sum())
        total += raw.numel()
    return {k: v / total for k, v in cnt.items()}


# ---- Philox jitter of the warp, restated in integers (csrc/common.h: philox2x32_10, key_mix; csrc/warp_device.h: jitter_point)
M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF
JITTER_STREAM = 0x554E


def philox2x32_10(c0, c1, key):
    """Philox2x32-10 on numpy uint64 arrays (or ints) holding 32-bit words -> (x, y)"""
    c0, c1 = np.asarray(c0, dtype=np.uint64), np.asarray(c1, dtype=np.uint64)
    k = int(key) & M32
    for _ in range(10):
        p = np.uint64(0xD256D193) * c0   # 32 x 32 -> 64 bits: no overflow
        c0, c1 = (p >> np.uint64(32)) ^ np.uint64(k) ^ c1, p & np.uint64(M32)
        k = (k + 0x9E3779B9) & M32
    return c0, c1


def key_mix(seed, iteration, stream):
    """32-bit key from the 64-bit seed, the stream id and the iteration bits above the 28 that the counter holds"""
    z = (int(seed) + 0x9E3779B97F4A7C15 * (int(stream) + 1) + (int(iteration) >> 28) * 0xD1B54A32D192ED03) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return (z ^ (z >> 32)) & M32


def philox_jitter_uniforms(seed, iteration, C, dims, Vg=None):
    """The U[0,1) draws jitter_point makes for (seed, iteration): (C,3,*dims) float32, each a 21-bit integer / 2^21.
    Counter (idx & 0xffffffff, (idx >> 32) | ((iteration << 4) & 0xffffffff)) with idx = chain * Vg + voxel, Vg = D*H*W of the
    whole volume; u0, u1 from the top 21 bits of the two output words, u2 from the 11 + 10 bits left below them."""
    V = int(np.prod(dims))
    Vg = V if Vg is None else int(Vg)
    idx = (np.arange(C, dtype=np.uint64)[:, None] * np.uint64(Vg) + np.arange(V, dtype=np.uint64)[None, :])
    c0 = idx & np.uint64(M32)
    c1 = (idx >> np.uint64(32)) | np.uint64((int(iteration) << 4) & M32)
    x, y = philox2x32_10(c0, c1, key_mix(seed, iteration, JITTER_STREAM))
    r = np.stack([x >> np.uint64(11), y >> np.uint64(11),
                  (x & np.uint64(0x7FF)) | ((y & np.uint64(0x3FF)) << np.uint64(11))], axis=1)   # (C,3,V), each < 2^21
    u = r.astype(np.float64) / 2097152.0
    return torch.from_numpy(u.astype(np.float32)).reshape(C, 3, *dims).contiguous()
