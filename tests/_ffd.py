"""Reference side of the cubic B-spline FFD pair irs_ffd_up / irs_ffd_adjoint (ffd_axis_kernel, csrc/field_kernels.hip), CPU only.

Matrix form.  Control point j of an axis with spacing c sits at the dense coordinate (j - 1) c, and tap i of the reference's
(4c - 1)-tap sampled spline (utils/transformation.py:79-102; centre tap r = 2c - 1) lies i - r voxels from it:
A[(j - 1) c + i - r, j] = k[i] wherever that row is inside [0, N) -- which is A[x, j] = beta3(x/c + 1 - j).  The entries are the
reference's float32-rounded taps cast to double; up64 = A_D (x) A_H (x) A_W applied axis by axis in float64, adj64 its transpose.
Nothing here goes through the kernel's gather indices nor through the oracle's conv_transpose1d and crop.

Tolerances (derived, not measured), u = 2^-24, gamma_n = n u / (1 - n u): up-sampling is three passes of at most four fused
multiply-adds, so |out - up64(v)| <= gamma_12 up64(|v|) element by element (the taps are >= 0: the envelope is the operator on
|v|); a control point of the adjoint sums at most min(4c - 1, N) rows per axis, so |out - adj64(g)| <= gamma_n adj64(|g|) with
n the sum of that over the axes.

Impulses.  A control-grid impulse of a power-of-two amplitude a at (j0, j1, j2) comes out as ((a kD) kH) kW, float32 products in the
order of the passes D, H, W, on the support [(j - 3) c + 1, (j + 1) c - 1] of each axis cut to the volume, and exactly +0 everywhere
else (every other term of an fmaf is 0 k).  A dense impulse goes through the adjoint as ((a kW) kH) kD at the at most 4^3 control points
that reach it."""
import math

import torch

from oracle import ops as O

F64 = torch.float64
U = 2.0 ** -24

# (D, H, W) / (c0, c1, c2), each the smallest shape that has its edge
CASES = [
    ((2, 3, 5), (8, 1, 2)),       # the smallest volume the ABI admits, N < cps, a 4-point control axis
    ((4, 4, 4), (2, 2, 2)),       # more scratch than 2 x (C,3,D,H,W) at cps 2
    ((16, 16, 16), (1, 1, 1)),    # the control grid is larger than the image
    ((9, 17, 33), (4, 8, 1)),     # (N - 1) % cps == 0 on every axis: the last row's fourth control point would be j = G; spacing 8
    ((8, 18, 34), (3, 5, 2)),     # (N - 1) % cps != 0 on every axis
]
IDS = ['x'.join(map(str, d)) + '-cps' + ''.join(map(str, c)) for d, c in CASES]
# where the two intermediates do not fit into 2 x (C,3,D,H,W)
OVERFLOWING = [((2, 3, 5), (8, 1, 2)), ((4, 4, 4), (2, 2, 2)), ((16, 16, 16), (1, 1, 1))]


def gamma(n):
    return n * U / (1.0 - n * U)


def grid(dims, cps):
    """ceil((N - 1) / cps) + 3 control points per axis, in integers"""
    return tuple((n - 1 + c - 1) // c + 3 for n, c in zip(dims, cps))


def axis_matrix(n, c):
    """A (n, G) float64: column j is the spline centred at (j - 1) c, sampled at the voxels 0 .. n - 1"""
    k = O.bspline_kernel_1d(c).to(F64)
    r = (k.numel() - 1) // 2
    G = grid((n,), (c,))[0]
    A = torch.zeros(n, G, dtype=F64)
    for j in range(G):
        for i in range(k.numel()):
            x = (j - 1) * c + i - r
            if 0 <= x < n:
                A[x, j] = k[i]
    return A


def matrices(dims, cps):
    return [axis_matrix(n, c) for n, c in zip(dims, cps)]


def _apply(t, mats, transpose):
    """every matrix (or its transpose) along its own axis of t (..., n0, n1, n2), in float64"""
    t = t.to(F64)
    for ax, A in zip((-3, -2, -1), mats):
        M = A.t() if transpose else A
        t = torch.tensordot(t, M, dims=([ax], [1])).movedim(-1, ax)
    return t


def up64(v, dims, cps):
    return _apply(v, matrices(dims, cps), False)


def adj64(g, cps):
    return _apply(g, matrices(g.shape[-3:], cps), True)


def up_bound(v, dims, cps):
    return gamma(12) * up64(v.abs(), dims, cps)


def adjoint_terms(dims, cps):
    return sum(min(4 * c - 1, n) for n, c in zip(dims, cps))


def adj_bound(g, cps):
    return gamma(adjoint_terms(g.shape[-3:], cps)) * adj64(g.abs(), cps)


# ------------------------------------------------------------------------------------------------ inputs
def scaled_normal(shape, seed):
    """N(0,1), channel 1 of every chain times 2^20 and channel 2 times 2^-20: no absolute tolerance fits all three"""
    t = torch.randn(*shape, generator=torch.Generator().manual_seed(seed))
    t[:, 1] *= 2.0 ** 20
    t[:, 2] *= 2.0 ** -20
    return t.contiguous()


def inputs(dims, cps, C, seed=0):
    """(v on the control grid, g on the volume), float32"""
    return scaled_normal((C, 3, *grid(dims, cps)), 2 * seed + 1), scaled_normal((C, 3, *dims), 2 * seed + 2)


# ------------------------------------------------------------------------------------------------ impulses
def control_picks(dims, cps):
    """per axis j in {0, 3, an interior point, G - 1}; 3 is the first point whose lower support edge (j - 3) c is in the volume"""
    return [sorted({0, 3, G // 2, G - 1}) for G in grid(dims, cps)]


def dense_picks(dims, cps):
    """per axis x in {0, c - 1, c, N - 1}, clamped to the volume"""
    return [sorted({min(x, n - 1) for x in (0, c - 1, c, n - 1)}) for n, c in zip(dims, cps)]


def batches(picks, slots=9):
    """the product of the per-axis picks in lists of `slots` positions (the last one filled up from the start)"""
    pos = [(a, b, c) for a in picks[0] for b in picks[1] for c in picks[2]]
    pos += pos[:(-len(pos)) % slots]
    return [pos[i:i + slots] for i in range(0, len(pos), slots)]


def impulses(shape3, positions, a):
    """(3,3,*shape3) float32 zeros with `a` at positions[3 chain + channel] of volume (chain, channel)"""
    t = torch.zeros(3, 3, *shape3)
    for s, p in enumerate(positions):
        t[s // 3, s % 3][p] = a
    return t


def expected_up(dims, cps, positions, a):
    """float32: ((a kD) kH) kW per (chain, channel), +0 off the support"""
    AD, AH, AW = (A.float() for A in matrices(dims, cps))
    out = torch.zeros(3, 3, *dims)
    for s, (j0, j1, j2) in enumerate(positions):
        e = (torch.tensor(a, dtype=torch.float32) * AD[:, j0]).view(-1, 1, 1)
        e = e * AH[:, j1].view(1, -1, 1)
        out[s // 3, s % 3] = e * AW[:, j2].view(1, 1, -1)
    return out


def expected_adj(dims, cps, positions, a):
    """float32: ((a kW) kH) kD per (chain, channel) on the control grid, +0 elsewhere"""
    AD, AH, AW = (A.float() for A in matrices(dims, cps))
    out = torch.zeros(3, 3, *grid(dims, cps))
    for s, (x0, x1, x2) in enumerate(positions):
        e = (torch.tensor(a, dtype=torch.float32) * AW[x2, :]).view(1, 1, -1)
        e = e * AH[x1, :].view(1, -1, 1)
        out[s // 3, s % 3] = e * AD[x0, :].view(-1, 1, 1)
    return out


def support(j, c, n):
    """[(j - 3) c + 1, (j + 1) c - 1] cut to [0, n)"""
    return max((j - 3) * c + 1, 0), min((j + 1) * c - 1, n - 1)


# ------------------------------------------------------------------------------------------------ scratch
def intermediates(C, dims, cps):
    """floats of the two intermediates of the three axis passes: up-sampling goes (G0,G1,G2) -> (D,G1,G2) -> (D,H,G2) -> (D,H,W), the
    adjoint the same way back; both arrays are alive while the middle pass runs"""
    D, H, W = dims
    _, G1, G2 = grid(dims, cps)
    return C * 3 * D * G1 * G2, C * 3 * D * H * G2


def scratch_floats(C, dims, cps):
    return sum(intermediates(C, dims, cps))


def old_contract_floats(C, dims):
    """2 x (C,3,D,H,W): what the header promised to be enough before irs_ffd_scratch_floats"""
    return 2 * C * 3 * math.prod(dims)
