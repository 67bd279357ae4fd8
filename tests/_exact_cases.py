"""Exact ("dyadic") inputs for the warp family, the Jacobian operators and the squaring steps with their adjoints, shared by the
host and GPU tests ("Numerics": the exact-case method), and an integer restatement of the Philox jitter of the warp.

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


# ---- squaring steps (csrc/exp_kernels.hip): d_out = d + sample(d, id + d) on a 3-channel field, and its adjoint
STEP_CLASSES = ('3/4', 'exactly 1', '7/4', 'exactly 2', 'past every face')   # the chains of a step case, by max|d| in voxels
STEP_REACH = (3, 4, 7, 8)            # quarter voxels: the amplitude of chains 0..3
STEP_WIDTHS = (1, 2, 2, 3)           # floor(max|d|) + 1 of chains 0..3; chain 4 is beyond 3


def extreme_voxels(dims):
    """[(z, y, x), sign] where the exact-amplitude classes hold +a or -a in all three channels.  For dims 2^k + 1 the last 32- or
    64-wide tile in x and the last 8-row tile in y hold one column / row: the far corner sits in the ragged last tile of both (the
    -a there points inwards and lands exactly a voxels inside, or on the near face where the axis is shorter than a), the origin
    on three faces (+a: inwards), the third on the face x = 0 (-a: outwards in x), the fourth in the ragged last tile row (+a:
    outwards in y)."""
    D, H, W = dims
    return [((D - 1, H - 1, W - 1), -1), ((0, 0, 0), 1), ((D // 2, H // 2, 0), -1), ((D // 2, H - 1, W // 2), 1)]


def dyadic_step_case(dims, seed=0):
    """One squaring step's input on which fp32 arithmetic is exact: D (5,3,*dims) in normalised units, = q * 2 / (n - 1) per axis
    with q on the quarter-voxel lattice, one chain per class of STEP_CLASSES: chains 0..3 white with |q| <= 3/4, 1, 7/4, 2 voxels
    (the bound held at extreme_voxels with both signs, whatever the draw), chain 4 with id + q anywhere up to 3 voxels past every
    face (_positions).  G (5,3,*dims): integers -8..8, the upstream gradient."""
    assert all(((n - 1) & (n - 2)) == 0 for n in dims), 'every dim must be 2^k + 1'
    g = torch.Generator().manual_seed(seed)
    q = torch.empty(5, 3, *dims, dtype=torch.float64)
    for chain, a in enumerate(STEP_REACH):
        q[chain] = torch.randint(-a, a + 1, (3, *dims), generator=g).double() / 4.0
        for (z, y, x), sign in extreme_voxels(dims):
            q[chain, :, z, y, x] = sign * a / 4.0
    for c, (n, idx) in enumerate(zip(axis_sizes(dims), _index_grids(dims))):
        q[4, c] = _positions(n, dims, 4, 3, g) - idx
    D = torch.stack([q[:, c] * (2.0 / (n - 1)) for c, n in enumerate(axis_sizes(dims))], 1)
    G = torch.randint(-8, 9, (5, 3, *dims), generator=g).float()
    assert torch.equal(D.float().double(), D)
    return SimpleNamespace(dims=tuple(dims), C=5, D=D.float().contiguous(), G=G)


def dyadic_velocity_case(dims, no_steps, reach, seed=0):
    """A velocity field v (len(reach),3,*dims) in VOXELS whose scaling-and-squaring chain of `no_steps` (1 or 2) steps is exact in
    fp32: v = q * 2^no_steps with q = d_0 on the quarter-voxel lattice for one step and on the half-voxel lattice for two
    ("Numerics note (exact cases)": why not finer, why not three steps).  reach[c] is chain c's: a number r (voxels, a
    multiple of the lattice step) draws q white in [-r, r], r held with both signs at extreme_voxels; ('checker', r), r <= 1/2,
    draws component c from {0, r (-1)^(index along c)}, 0 where that would point out of the volume.  Where such a component is not
    0 its sample sits between two neighbours along c that are 0 or of opposite sign, |sample| <= r (1 - r); where it is 0 the sample
    is one of the field's values or a mean of them along the other axes, at most r: max|d_1| <= max(r (2 - r), r) = 3/4 voxel
    for r = 1/2 -- on the half-voxel lattice, where white noise of the smallest amplitude reaches |d_1| = 1, the way to keep a
    chain's d_1 inside the radius-1 ring."""
    assert no_steps in (1, 2) and all(((n - 1) & (n - 2)) == 0 for n in dims), 'every dim must be 2^k + 1'
    step = 4 if no_steps == 1 else 2
    g = torch.Generator().manual_seed(seed)
    q = torch.empty(len(reach), 3, *dims, dtype=torch.float64)
    for chain, r in enumerate(reach):
        checker = isinstance(r, tuple)
        a = (r[1] if checker else r) * step
        assert a == int(a) and a >= 1, 'a reach is a multiple of the lattice step'
        a = int(a)
        if checker:
            sign = torch.stack([(1.0 - 2.0 * (idx % 2)) * (idx + 1 - 2 * (idx % 2) <= n - 1)
                                for idx, n in zip(_index_grids(dims), axis_sizes(dims))]).double()
            q[chain] = torch.randint(0, 2, (3, *dims), generator=g).double() * sign * (a / step)
        else:
            q[chain] = torch.randint(-a, a + 1, (3, *dims), generator=g).double() / step
            for (z, y, x), s in extreme_voxels(dims):
                q[chain, :, z, y, x] = s * a / step
    v = q * float(2 ** no_steps)
    assert torch.equal(v.float().double(), v)
    return SimpleNamespace(dims=tuple(dims), C=len(reach), no_steps=no_steps, v=v.float().contiguous())


# ---- the cases the GPU tests run; tests/test_exact_cases_host.py proves fp32 == fp64 on each of them
VELOCITY_CASES = {   # name -> (no_steps, reach per chain in voxels of d_0)
    'one step': (1, (0.25, 0.75, 1, 3)),                          # max|d_0| 1/4, 3/4, 1, 3
    'two steps': (2, (('checker', 0.5), 0.5, 1, 3)),              # max|d_1| < 1, in [1, 2), >= 2, >= 2; max|d_2| towards 12
    'two steps, far': (2, (0.5, 6)),                              # max|d_2| towards 24 voxels
    'engine': (2, (('checker', 0.5), 0.5, 3)),                    # max|d_1| < 1, in [1, 2), >= 2
}


def step_case(dims):
    return dyadic_step_case(dims, seed=4000 + EXACT_DIMS.index(tuple(dims)))


def velocity_case(dims, name):
    no_steps, reach = VELOCITY_CASES[name]
    return dyadic_velocity_case(dims, no_steps, reach, seed=5000 + 10 * EXACT_DIMS.index(tuple(dims)) + list(VELOCITY_CASES).index(name))


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


def step_reference(d, G, dtype, explicit=False):
    """One squaring step d_out = d + sample(d, id + d) and its adjoint on a field d (C,3,*dims) in normalised units, in `dtype`:
    -> (d_out, d(sum(d_out * G)) / d(d)).  Through ATen's grid_sample and autograd, or (explicit) restated with the oracle's own
    sampler and its two adjoints, which share no arithmetic with ATen or the kernels: G itself, the trilinear scatter of G (the
    gradient w.r.t. the sampled field) and the coordinate gradient (w.r.t. the sampling grid), which _unnormalise_clip switches
    off unless the coordinate is strictly inside the volume."""
    dims = tuple(d.shape[2:])
    d, G = d.to(dtype), G.to(dtype)
    if explicit:
        g5 = (identity(dims, dtype) + d).permute(0, 2, 3, 4, 1)
        out = d + O.trilinear_sample_explicit(d, g5)
        g_field, g_grid = O.trilinear_backward_explicit(d, g5, G)
        return out, G + g_field + g_grid.permute(0, 4, 1, 2, 3)
    d = d.clone().requires_grad_(True)
    out = d + O.warp_trilinear(d, identity(dims, dtype) + d)
    gd, = torch.autograd.grad(out, d, G)
    return out.detach(), gd


def chain_reference(v, no_steps, dtype, g_last=None):
    """O.svf_exp of a velocity field in voxels, in `dtype`: -> (transformation, displacement, [d_0 .. d_n], grad_v or None), grad_v
    = d(sum(d_n * g_last)) / d(v) by autograd"""
    v = v.to(dtype).clone().requires_grad_(g_last is not None)
    t, disp, steps = O.svf_exp(v, no_steps, keep_steps=True)
    gv = None
    if g_last is not None:
        gv, = torch.autograd.grad(steps[-1], v, g_last.to(dtype))
    return t.detach(), disp.detach(), [s.detach() for s in steps], gv


def step_widths(d):
    """floor(max|d|) + 1 per chain of a field (C,3,*dims) in normalised units, |d| in voxels and the maximum over the three axes:
    what the device decides the kernel of a step by (1: radius-1 ring / gather, 2: radius-2, 3 and more: global-memory taps /
    the any-radius adjoint)"""
    vox = O.to_voxels(d.double()).abs().flatten(1).max(1).values
    return [int(m) + 1 for m in vox.tolist()]


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
