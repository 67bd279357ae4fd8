"""Restatement of the inverse-consistency operators in torch at a given dtype, shared by the host and GPU tests: the
composition r = d_a + trilinear(d_b)(t_a) with the oracle's sampler, its norm, and the Welford / peak update of the norm maps.
Inputs are CPU tensors; `dtype` is torch.float32 or torch.float64."""
import torch

from oracle import ops as O
from tests import _exact_cases as X


def smooth_field(C, dims, amp, seed):
    """a smooth random velocity field (C,3,*dims) in voxel units: white noise of amplitude `amp` under the Sobolev kernel"""
    g = torch.Generator().manual_seed(seed)
    return O.separable_conv3d_replicate(amp * torch.randn(C, 3, *dims, generator=g), O.sobolev_kernel_1d(3, 0.5)).contiguous()


def compose(t_a, d_a, d_b, dtype, scale=(1.0, 1.0, 1.0)):
    """-> (residual (C,3,D,H,W), norm (C,1,D,H,W)) in `dtype`: r = d_a + trilinear(d_b)(t_a), norm = sqrt(sum_c (scale_c r_c)^2)
    with the sum taken in channel order"""
    r = d_a.to(dtype) + O.warp_trilinear(d_b.to(dtype), t_a.to(dtype))
    s = [r[:, c:c + 1] * torch.tensor(scale[c], dtype=dtype) for c in range(3)]
    return r, torch.sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2])


def tap_weight_sum(t_a, d_b):
    """sum over the eight taps of |w v| per channel, (C,3,D,H,W) float64: what the rounding of the products and of their sum
    scales with"""
    return O.warp_trilinear(d_b.double().abs(), t_a.double())


def chain_summary(norm, mask=None):
    """one chain's summary columns from its norm map (D,H,W): ([voxels, non-finite], [sum, sum of squares, max]) in float64 over
    the mask (bool (D,H,W) or None); the maximum of nothing is -inf"""
    x = norm.double().reshape(-1)
    if mask is not None:
        x = x[mask.reshape(-1).bool()]
    fin = x[torch.isfinite(x)]
    return ([int(x.numel()), int(x.numel() - fin.numel())],
            [float(fin.sum()), float((fin * fin).sum()), float(fin.max()) if fin.numel() else float('-inf')])


def update(state, norm, records_before, dtype):
    """fold the C maps of norm (C,1,D,H,W) into state = (mean, peak) (each (D,H,W) in `dtype`, or None before the first record)
    in chain order: mean += (x - mean) / k with k = records_before + c + 1 (k = 1: mean = x); peak = max(peak, x) over the
    finite x only, NaN where none was finite.  records_before = 0 ignores the state.  -> (mean, peak)"""
    norm = norm.to(dtype)
    mean, peak = (None, None) if records_before == 0 or state is None else state
    for c in range(norm.shape[0]):
        x = norm[c, 0]
        k = records_before + c + 1
        if k == 1:
            mean, peak = x.clone(), torch.full_like(x, float('nan'))
        else:
            mean = mean + (x - mean) / torch.tensor(float(k), dtype=dtype)
        fin = torch.isfinite(x)
        peak = torch.where(fin, torch.where(torch.isnan(peak), x, torch.maximum(peak, torch.where(fin, x, peak))), peak)
    return mean, peak


def map_summary(mean, peak, threshold, mask=None):
    """the finalize's columns from the two maps: ([voxels, non-finite mean, peak > threshold], [sum mean, max mean, max peak])"""
    m, p = mean.double().reshape(-1), peak.double().reshape(-1)
    if mask is not None:
        keep = mask.reshape(-1).bool()
        m, p = m[keep], p[keep]
    mf, pf = m[torch.isfinite(m)], p[torch.isfinite(p)]
    ninf = float('-inf')
    return ([int(m.numel()), int(m.numel() - mf.numel()), int((pf > threshold).sum())],
            [float(mf.sum()), float(mf.max()) if mf.numel() else ninf, float(pf.max()) if pf.numel() else ninf])


# ---- the exact cases of the composition (tests/test_inverse_consistency_host.py proves fp32 == fp64 on each of them)
def exact_case(dims):
    """t_a = identity + d_last and d_a = d_last of the dyadic warp case (positions on the quarter-voxel lattice, reaching three
    voxels past every face); d_b: integers in -8..8 divided by 4.  -> (t_a, d_a, d_b), each (CHAINS,3,*dims) float32"""
    case = X.warp_case(dims, False)
    t_a = (X.identity(dims) + case.d_last).contiguous()
    g = torch.Generator().manual_seed(4000 + X.EXACT_DIMS.index(tuple(dims)))
    d_b = torch.randint(-8, 9, (case.C, 3, *dims), generator=g).float() / 4.0
    return t_a, case.d_last, d_b


def exact_masks(dims, C):
    """a mask shared by the chains (1,1,*dims) and one per chain (C,1,*dims), bool, about half set"""
    g = torch.Generator().manual_seed(5000 + X.EXACT_DIMS.index(tuple(dims)))
    m = torch.rand(C, 1, *dims, generator=g) > 0.5
    return m[:1].contiguous(), m
