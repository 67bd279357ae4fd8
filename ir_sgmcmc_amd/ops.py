"""Functional wrappers over the stateless C-ABI operators (torch tensors in, torch tensors out, GPU only).

Each function names the reference call it stands in for; the classes in `ir_sgmcmc_amd.utils` / `.model` that mirror
the reference's modules are thin shells over these.
"""
import ctypes as C
import math
import statistics
from collections import namedtuple

import numpy as np
import torch

from . import _lib as L


# ---- what the operators below share: the call itself, then one copy of every check, table and buffer set-up
def _call(name, *args):
    """the C-ABI operator `name` on the current stream, its arguments in header order; a refusal raises with irs_last_error()"""
    L.check(getattr(L.load(), name)(*args, L.stream_ptr()))


def _workspace(query, *args, device):
    """(uint8 workspace on the device, its size in bytes) as the size query `query`(*args, &bytes) of an operator wants it"""
    nbytes = C.c_size_t()
    L.check(getattr(L.load(), query)(*args, C.byref(nbytes)))
    return torch.empty(nbytes.value, device=device, dtype=torch.uint8), nbytes.value


def _summary_buffers(ws_bytes, ints, floats, device):
    """(ws, isummary, fsummary) of a finalizer: its fixed-size workspace and its int64 / float64 summaries of the given shapes"""
    return (torch.empty(ws_bytes, device=device, dtype=torch.uint8), torch.empty(ints, device=device, dtype=torch.int64),
            torch.empty(floats, device=device, dtype=torch.float64))


def _dims5(t, ch=None):
    if t.dim() != 5 or (ch is not None and t.shape[1] != ch):
        raise L.IrsError(f'expected a (C,{ch if ch else "ch"},D,H,W) tensor, got {tuple(t.shape)}')
    return t.shape[0], t.shape[2], t.shape[3], t.shape[4]


def _is_chain_volumes(t, Cn, D, H, W, shared_ok=True):
    """(Cn,1,D,H,W) -- or (1,1,D,H,W), one volume shared by the chains, where the ABI takes a chain count for it"""
    return t.dim() == 5 and t.shape[1] == 1 and t.shape[0] in ((1, Cn) if shared_ok else (Cn,)) and tuple(t.shape[2:]) == (D, H, W)


def _chain_volumes(name, t, like_name, Cn, D, H, W, shared_ok=True):
    if not _is_chain_volumes(t, Cn, D, H, W, shared_ok):
        raise L.IrsError(f'{name} shape {tuple(t.shape)} does not match {like_name}: '
                         f'({"1 or " if shared_ok else ""}{Cn},1,{D},{H},{W}) expected')


def _check_state(*rows):
    """rows of (name, tensor, shape, dtype): the first tensor of another shape or dtype is refused; dtype None leaves the dtype
    to dev_ptr"""
    for name, t, shape, dtype in rows:
        if tuple(t.shape) == tuple(shape) and dtype in (None, t.dtype):
            continue
        if dtype is None:
            raise L.IrsError(f'{name} must have shape {tuple(shape)}, got {tuple(t.shape)}')
        raise L.IrsError(f'{name} must be a {tuple(shape)} {dtype} tensor, got {t.dtype} {tuple(t.shape)}')


def _as_uint8(mask):
    """a bool / uint8 mask as the contiguous uint8 tensor the C ABI reads"""
    mask = mask.contiguous()
    return mask.view(torch.uint8) if mask.dtype == torch.bool else mask


def _volume_mask(mask, D, H, W):
    """mask of D H W elements, whatever its leading dimensions, or None"""
    if mask is None:
        return None
    if mask.numel() != D * H * W or mask.dtype not in (torch.bool, torch.uint8):
        raise L.IrsError(f'mask must be a bool / uint8 ({D},{H},{W}) volume, got {mask.dtype} {tuple(mask.shape)}')
    return _as_uint8(mask.reshape(D, H, W))


def _shared_mask(mask, D, H, W):
    """mask of exactly (1,1,D,H,W), shared by the chains, or None"""
    if mask is None:
        return None
    if tuple(mask.shape) != (1, 1, D, H, W) or mask.dtype not in (torch.bool, torch.uint8):
        raise L.IrsError(f'mask must be a bool / uint8 (1,1,{D},{H},{W}) volume, got {mask.dtype} {tuple(mask.shape)}')
    return _as_uint8(mask)


def _labels(labels):
    """(c_int32 table of the label values, never empty as a C array; how many it holds)"""
    labels = [int(x) for x in labels]
    return (C.c_int32 * max(len(labels), 1))(*labels), len(labels)


def _three_floats(values, refusal, ok=None):
    """values (a sequence, an array or a tensor) as the float[3] of the C ABI; refusal(values) words the error for another
    count, or for a value that `ok` does not hold for"""
    values = [float(v) for v in (values.tolist() if hasattr(values, 'tolist') else values)]
    if len(values) != 3 or not (ok is None or all(ok(v) for v in values)):
        raise L.IrsError(refusal(values))
    return (C.c_float * 3)(*values)


def _three_positive(name, values):
    return _three_floats(values, lambda v: f'{name} must hold three finite floats > 0, got {v}', lambda v: math.isfinite(v) and v > 0)


# `boxes` points into `boxes_host`: whoever passes `boxes` to the C ABI holds the whole tuple until that call has returned
_Contours = namedtuple('_Contours', 'labels n_labels spacing boxes boxes_host ws ws_bytes')


def _contour_setup(f, fixed_chains, m, labels, spacing, workspace, Cn, D, H, W, device):
    """What the contour-distance operators do before their own call.  f, m: the device pointers of the fixed (fixed_chains of
    them) and the moving segmentation; workspace(boxes, n_pairs) -> (ws, bytes): the operator's own size query.  -> _Contours:
    the label table and its length, the spacing as float[3], the bounding box of every (chain, label) pair -- computed on the
    device, read back once, as the int32 host pointer the C ABI takes --, and the workspace those boxes ask for."""
    lab, n = _labels(labels)
    sp = _three_floats(spacing, lambda v: f'spacing must have 3 entries, got {len(v)}')
    P = Cn * n
    boxes = torch.empty((max(P, 1), 6), device=device, dtype=torch.int32)
    _call('irs_label_boxes', f, fixed_chains, m, lab, n, L.dev_ptr(boxes), Cn, D, H, W)
    boxes_host = boxes.cpu()
    bp = C.cast(C.c_void_p(boxes_host.data_ptr()), C.POINTER(C.c_int32))
    return _Contours(lab, n, sp, bp, boxes_host, *workspace(bp, P))


def sobolev_kernel_1d(s, lam):
    """Normalised middle column of (I - lambda L)^-1, L the (2s+1)-point 1-D Laplacian
    (reference utils/functions.py:24-49, where it is read off an eigendecomposition)."""
    n = 2 * s + 1
    lap = -2.0 * np.eye(n) + np.eye(n, k=1) + np.eye(n, k=-1)
    e = np.zeros(n)
    e[s] = 1.0
    col = np.linalg.solve(np.eye(n) - lam * lap, e)
    return (col / col.sum()).astype(np.float32)


def control_grid_size(dims, cps):
    """utils/util.py:61-69"""
    return tuple(int(math.ceil((n - 1) / c) + 1 + 2) for n, c in zip(dims, cps))


def perturb_smooth(v, kernel, sigma=None, eps=None, tau=None, seed=0, iteration=0):
    """SGLD.forward (+ injected or Philox noise) followed by SobolevGrad.forward
    (utils/functions.py:76-109).  tau=None -> smoothing only; kernel=None -> perturbation only."""
    Cn, D, H, W = _dims5(v, 3)
    out = torch.empty_like(v)
    s = 0 if kernel is None else (len(kernel) - 1) // 2
    tmp = torch.empty_like(v) if s > 0 else None
    k = (C.c_float * (2 * s + 1))(*[float(x) for x in kernel]) if s > 0 else None
    _call('irs_perturb_smooth', L.dev_ptr(v, torch.float32), L.dev_ptr(sigma, torch.float32, True),
          L.dev_ptr(eps, torch.float32, True), -1.0 if tau is None else float(tau),
          C.cast(k, C.c_void_p) if k is not None else None, s, Cn, D, H, W, L.dev_ptr(tmp, None, True), L.dev_ptr(out), seed,
          iteration)
    return out


def svf_exp_fwd(v, no_steps=12, want_outputs=True):
    """SVF_3D.forward (utils/transformation.py:63-76).  Returns (transformation, displacement, steps)."""
    Cn, D, H, W = _dims5(v, 3)
    steps = torch.empty((no_steps,) + tuple(v.shape), device=v.device, dtype=torch.float32)
    t = torch.empty_like(v) if want_outputs else None
    d = torch.empty_like(v) if want_outputs else None
    _call('irs_svf_exp_fwd', L.dev_ptr(v, torch.float32), L.dev_ptr(steps), L.dev_ptr(t, None, True), L.dev_ptr(d, None, True),
          no_steps, Cn, D, H, W)
    return t, d, steps


def svf_exp_bwd(v, steps, g_last):
    """Gradient w.r.t. v of the scaling-and-squaring chain given dL/d(d_last) in normalised units."""
    Cn, D, H, W = _dims5(v, 3)
    scratch = torch.empty((2,) + tuple(v.shape), device=v.device, dtype=torch.float32)
    g_v = torch.empty_like(v)
    _call('irs_svf_exp_bwd', L.dev_ptr(v, torch.float32), L.dev_ptr(steps, torch.float32),
          L.dev_ptr(g_last.contiguous(), torch.float32), L.dev_ptr(scratch), L.dev_ptr(g_v), steps.shape[0], Cn, D, H, W)
    return g_v


def _ffd_scratch(Cn, D, H, W, cps, device):
    """the scratch of irs_ffd_up / irs_ffd_adjoint, sized by irs_ffd_scratch_floats (0: arguments the operators refuse)"""
    floats = L.load().irs_ffd_scratch_floats(Cn, D, H, W, *cps)
    if floats == 0:
        raise L.IrsError(f'ffd: dims {(D, H, W)} x {Cn} chains / cps {tuple(cps)} are refused (every extent >= 2, spacings 1..8)')
    return torch.empty(floats, device=device, dtype=torch.float32)


def ffd_up(v_cp, dims, cps):
    """Cubic_B_spline_FFD_3D.forward (utils/transformation.py:146-153)."""
    Cn = v_cp.shape[0]
    D, H, W = dims
    if tuple(v_cp.shape[2:]) != control_grid_size(dims, cps):
        raise L.IrsError(f'control grid {tuple(v_cp.shape[2:])} does not match dims {dims} / cps {cps}')
    dense = torch.empty((Cn, 3, D, H, W), device=v_cp.device, dtype=torch.float32)
    tmp = _ffd_scratch(Cn, D, H, W, cps, v_cp.device)
    _call('irs_ffd_up', L.dev_ptr(v_cp, torch.float32), L.dev_ptr(dense), L.dev_ptr(tmp), Cn, D, H, W, *cps)
    return dense


def ffd_adjoint(g_dense, cps):
    Cn, D, H, W = _dims5(g_dense, 3)
    G = control_grid_size((D, H, W), cps)
    g_cp = torch.empty((Cn, 3, *G), device=g_dense.device, dtype=torch.float32)
    tmp = _ffd_scratch(Cn, D, H, W, cps, g_dense.device)
    _call('irs_ffd_adjoint', L.dev_ptr(g_dense.contiguous(), torch.float32), L.dev_ptr(g_cp), L.dev_ptr(tmp), Cn, D, H, W, *cps)
    return g_cp


def _jitter_draws(unif, d_last):
    if unif is not None and tuple(unif.shape) != tuple(d_last.shape):
        raise L.IrsError(f'unif shape {tuple(unif.shape)} does not match d_last {tuple(d_last.shape)}')


def warp_displacement(im, d_last, unif=None, alpha=0.0, seed=0, iteration=0):
    """Trilinear warp at id + d_last (+ uniform jitter): registration_module(im, transformation_with_noise)."""
    Cn, D, H, W = _dims5(d_last, 3)
    _chain_volumes('image', im, 'd_last', Cn, D, H, W)
    _jitter_draws(unif, d_last)
    out = torch.empty((Cn, 1, D, H, W), device=d_last.device, dtype=torch.float32)
    _call('irs_warp_fwd', L.dev_ptr(im, torch.float32), im.shape[0], L.dev_ptr(d_last, torch.float32),
          L.dev_ptr(unif, torch.float32, True), float(alpha), L.dev_ptr(out), Cn, D, H, W, seed, iteration)
    return out


def warp_displacement_bwd(im, d_last, g_warped, unif=None, alpha=0.0, seed=0, iteration=0):
    Cn, D, H, W = _dims5(d_last, 3)
    _chain_volumes('image', im, 'd_last', Cn, D, H, W)
    _chain_volumes('g_warped', g_warped, 'd_last', Cn, D, H, W, shared_ok=False)
    _jitter_draws(unif, d_last)
    g_d = torch.empty_like(d_last)
    _call('irs_warp_bwd', L.dev_ptr(im, torch.float32), im.shape[0], L.dev_ptr(d_last, torch.float32),
          L.dev_ptr(unif, torch.float32, True), float(alpha), L.dev_ptr(g_warped.contiguous(), torch.float32), L.dev_ptr(g_d),
          Cn, D, H, W, seed, iteration)
    return g_d


_WARP_ENTRY = {torch.float32: 'irs_warp_transformation', torch.bool: 'irs_warp_nearest_u8', torch.int16: 'irs_warp_nearest_i16'}


def warp(im, transformation):
    """RegistrationModule.forward (utils/registration.py:17-32): float -> trilinear; bool / int16 -> nearest."""
    Cn, D, H, W = _dims5(transformation, 3)
    if not _is_chain_volumes(im, Cn, D, H, W):
        raise L.IrsError(f'image shape {tuple(im.shape)} does not match transformation {tuple(transformation.shape)}')
    t = L.dev_ptr(transformation, torch.float32)
    if im.dtype not in _WARP_ENTRY:
        raise NotImplementedError  # same error behaviour as utils/registration.py:32
    out = torch.empty((Cn, 1, D, H, W), device=im.device, dtype=im.dtype)
    _call(_WARP_ENTRY[im.dtype], L.dev_ptr(im), im.shape[0], t, L.dev_ptr(out), Cn, D, H, W)
    return out


def lcc_normalise(im, s, want_sigma=False):
    """(I - u) / sqrt(var + 1e-10) with (2s+1)^3 replicate-padded box statistics (model/loss.py:103-109)."""
    Cn, D, H, W = _dims5(im, 1)
    out = torch.empty_like(im)
    sig = torch.empty_like(im) if want_sigma else None
    _call('irs_lcc_normalise', L.dev_ptr(im, torch.float32), L.dev_ptr(out), L.dev_ptr(sig, None, True), s, Cn, D, H, W)
    return (out, sig) if want_sigma else out


def lcc_map_fwd(fhat, warped, s):
    Cn, D, H, W = _dims5(warped, 1)
    _chain_volumes('fhat', fhat, 'warped', Cn, D, H, W)
    z = torch.empty_like(warped)
    sig = torch.empty_like(warped)
    _call('irs_lcc_map_fwd', L.dev_ptr(fhat, torch.float32), fhat.shape[0], L.dev_ptr(warped, torch.float32), L.dev_ptr(z),
          L.dev_ptr(sig), s, Cn, D, H, W)
    return z, sig


def lcc_map_bwd(fhat, z, sigma_m, g_z, s):
    Cn, D, H, W = _dims5(z, 1)
    _chain_volumes('fhat', fhat, 'z', Cn, D, H, W)
    _chain_volumes('sigma_m', sigma_m, 'z', Cn, D, H, W, shared_ok=False)
    _chain_volumes('g_z', g_z, 'z', Cn, D, H, W, shared_ok=False)
    g = torch.empty_like(z)
    _call('irs_lcc_map_bwd', L.dev_ptr(fhat, torch.float32), fhat.shape[0], L.dev_ptr(z, torch.float32),
          L.dev_ptr(sigma_m, torch.float32), L.dev_ptr(g_z.contiguous(), torch.float32), L.dev_ptr(g), s, Cn, D, H, W)
    return g


def reg_energy(v):
    """sum of squared replicate-padded forward differences per chain (model/loss.py:158-159) -> (C,) float64"""
    Cn, D, H, W = _dims5(v, 3)
    y = torch.empty(Cn, device=v.device, dtype=torch.float64)
    scratch = torch.empty(L.load().irs_reduce_scratch_doubles(), device=v.device, dtype=torch.float64)
    _call('irs_reg_energy', L.dev_ptr(v, torch.float32), L.dev_ptr(y), L.dev_ptr(scratch), Cn, D, H, W)
    return y


def gradient_operator(v, transformation=False):
    """GradientOperator.forward (utils/diff_op.py:78-96) -> (C,3,D,H,W,3)"""
    Cn, D, H, W = _dims5(v, 3)
    nabla = torch.empty((Cn, 3, D, H, W, 3), device=v.device, dtype=torch.float32)
    _call('irs_gradient_operator', L.dev_ptr(v, torch.float32), L.dev_ptr(nabla), int(bool(transformation)), Cn, D, H, W)
    return nabla


def log_det_jacobian(transformation):
    """calc_no_non_diffeomorphic_voxels (utils/util.py:209-212): (NaN count per chain as int64 tensor, log det J)"""
    Cn, D, H, W = _dims5(transformation, 3)
    ld = torch.empty((Cn, D, H, W), device=transformation.device, dtype=torch.float32)
    cnt = torch.empty(Cn, device=transformation.device, dtype=torch.int64)
    _call('irs_log_det_jacobian', L.dev_ptr(transformation, torch.float32), L.dev_ptr(ld), L.dev_ptr(cnt), Cn, D, H, W)
    return cnt, ld


def _average_distance(counts, sums):
    """(P,2) contour sizes and directed distance sums -> (P,) mean of the two directed averages, inf where a contour is empty"""
    empty = (counts == 0).any(dim=1)
    asd = 0.5 * (sums[:, 0] / counts[:, 0].clamp(min=1) + sums[:, 1] / counts[:, 1].clamp(min=1))
    return torch.where(empty, torch.full_like(asd, math.inf), asd)


def label_surface_distance(seg_fixed, seg_moving, labels, spacing):
    """Average surface distance per chain and label, the ASD half of calc_metrics (utils/util.py:152-206): contours as
    sitk.LabelContour draws them (face neighbours inside the volume), GetAverageHausdorffDistance of the two contours with an
    exact Euclidean distance transform.  seg_fixed (Cf,1,D,H,W) int16 with Cf in {1, C}, seg_moving (C,1,D,H,W) int16,
    spacing (sx, sy, sz) as SetSpacing takes it (sx scales the last axis).  -> (C, L) float64 tensor; inf where a contour
    is empty (the reference's `except` branch).  One device-to-host read: the boxes that size the workspace."""
    Cn, D, H, W = _dims5(seg_moving, 1)
    if not _is_chain_volumes(seg_fixed, Cn, D, H, W):
        raise L.IrsError(f'fixed segmentation {tuple(seg_fixed.shape)} does not match the moving one {tuple(seg_moving.shape)}')
    f, m = L.dev_ptr(seg_fixed, torch.int16), L.dev_ptr(seg_moving, torch.int16)
    dev = seg_moving.device
    c = _contour_setup(f, seg_fixed.shape[0], m, labels, spacing,
                       lambda boxes, P: _workspace('irs_surface_distance_workspace', boxes, P, D, H, W, device=dev), Cn, D, H, W, dev)
    P = Cn * c.n_labels
    counts = torch.empty((P, 2), device=dev, dtype=torch.int64)
    sums = torch.empty((P, 2), device=dev, dtype=torch.float64)
    _call('irs_label_surface_distance', f, seg_fixed.shape[0], m, c.labels, c.n_labels, c.spacing, c.boxes, L.dev_ptr(c.ws),
          c.ws_bytes, L.dev_ptr(counts), L.dev_ptr(sums), Cn, D, H, W)
    return _average_distance(counts, sums).view(Cn, c.n_labels)


def label_hausdorff_distance(seg_fixed, seg_moving, labels, spacing, percentiles=(95,)):
    """Hausdorff and percentile surface distances per chain and label, next to the ASD of label_surface_distance, from the same
    contours and the same exact distance transform (absent in the reference; sitk's GetHausdorffDistance is the maximum).
    Arguments as label_surface_distance; percentiles: 0 to 4 strictly increasing values in (0, 100].  The directed percentile q
    of the n distances of one contour to the other is their ascending order statistic of 0-based index
    min(max(ceil(q * n / 100) - 1, 0), n - 1) (numpy's method='inverted_cdf'), selected exactly on the device.
    -> dict of float64 device tensors: 'asd' (C, L), bit-identical to label_surface_distance; 'hd' (C, L) and 'hd_directed'
    (C, L, 2) ([..., 0]: max over the fixed contour of the distance to the moving one, [..., 1]: the reverse); 'hd_pct'
    (Q, C, L) and 'hd_pct_directed' (Q, C, L, 2).  The symmetric values are the larger of the two directions; everything is
    inf where a contour is empty.  One device-to-host read: the boxes that size the workspace."""
    Cn, D, H, W = _dims5(seg_moving, 1)
    if not _is_chain_volumes(seg_fixed, Cn, D, H, W):
        raise L.IrsError(f'fixed segmentation {tuple(seg_fixed.shape)} does not match the moving one {tuple(seg_moving.shape)}')
    f, m = L.dev_ptr(seg_fixed, torch.int16), L.dev_ptr(seg_moving, torch.int16)
    pct = [float(x) for x in percentiles]
    Q = len(pct)
    dev = seg_moving.device
    c = _contour_setup(f, seg_fixed.shape[0], m, labels, spacing,
                       lambda boxes, P: _workspace('irs_hausdorff_workspace', boxes, P, Q, D, H, W, device=dev), Cn, D, H, W, dev)
    n, P = c.n_labels, Cn * c.n_labels
    counts = torch.empty((P, 2), device=dev, dtype=torch.int64)
    sums = torch.empty((P, 2), device=dev, dtype=torch.float64)
    hd = torch.empty((P, 2), device=dev, dtype=torch.float64)
    hd_pct = torch.empty((Q, P, 2), device=dev, dtype=torch.float64)
    _call('irs_label_hausdorff_distance', f, seg_fixed.shape[0], m, c.labels, n, c.spacing, c.boxes, L.dev_ptr(c.ws), c.ws_bytes,
          (C.c_double * max(Q, 1))(*pct), Q, L.dev_ptr(counts), L.dev_ptr(sums), L.dev_ptr(hd), L.dev_ptr(hd_pct) if Q else None,
          Cn, D, H, W)
    return {'asd': _average_distance(counts, sums).view(Cn, n),
            'hd': hd.max(dim=1).values.view(Cn, n), 'hd_directed': hd.view(Cn, n, 2),
            'hd_pct': hd_pct.max(dim=2).values.view(Q, Cn, n), 'hd_pct_directed': hd_pct.view(Q, Cn, n, 2)}


SURFACE_INT_COLUMNS = ('contour_voxels', 'sampled_voxels', 'spread_voxels')  # then one column per coverage level
SURFACE_FLOAT_COLUMNS = ('bias_sum', 'abs_bias_sum', 'bias_sq_sum', 'abs_bias_max', 'std_sum', 'std_max')


def _surface_state(mean, m2, count, shape):
    _check_state(('mean', mean, shape, torch.float32), ('m2', m2, shape, torch.float32), ('count', count, shape, torch.int32))


def surface_posterior_update(seg_fixed, seg_moving, labels, spacing, mean, m2, count):
    """Fold one recorded step into the surface posterior (absent in the reference).  seg_fixed (1,1,D,H,W) int16, the fixed
    segmentation the chains share; seg_moving (C,1,D,H,W) int16, every chain's warped segmentation; labels: 1 to 64 distinct
    values; spacing (sx, sy, sz) as label_surface_distance takes it; mean / m2 (D,H,W) float32 and count (D,H,W) int32, zero
    before the first step, updated in place.  At every voxel of the fixed contour of a listed label each chain whose map holds
    the label gives the sample s = sign * distance to the nearest voxel of the label's contour in that chain's map, the
    distances of label_hausdorff_distance; sign -1 where the chain's map has the label at the voxel (the fixed surface lies
    inside the warped structure: the structure came out too large there), +1 otherwise; 0 on the moving contour itself.  The
    samples enter the Welford moments in chain order: include/irsgmcmc.h has the recurrence.  Other voxels are never touched.
    One device-to-host read: the boxes that size the workspace."""
    Cn, D, H, W = _dims5(seg_moving, 1)
    if tuple(seg_fixed.shape) != (1, 1, D, H, W):
        raise L.IrsError(f'fixed segmentation {tuple(seg_fixed.shape)} does not match the moving one {tuple(seg_moving.shape)}: '
                         f'(1,1,{D},{H},{W}) expected')
    _surface_state(mean, m2, count, (D, H, W))
    f, m = L.dev_ptr(seg_fixed, torch.int16), L.dev_ptr(seg_moving, torch.int16)
    ptrs = [L.dev_ptr(t) for t in (mean, m2, count)]
    dev = seg_moving.device
    c = _contour_setup(f, 1, m, labels, spacing,
                       lambda boxes, P: _workspace('irs_surface_posterior_workspace', boxes, P, D, H, W, device=dev), Cn, D, H, W, dev)
    _call('irs_surface_posterior_update', f, m, c.labels, c.n_labels, c.spacing, c.boxes, L.dev_ptr(c.ws), c.ws_bytes, *ptrs,
          Cn, D, H, W)


def surface_posterior_finalize(seg_fixed, labels, mean, m2, count, levels, mask=None):
    """The maps and the per-label summary of the surface posterior (absent in the reference).  seg_fixed (1,1,D,H,W) int16; the
    state of surface_posterior_update; levels: 0 to 4 strictly increasing coverage levels in (0, 1); mask (D,H,W) bool / uint8
    or None.  -> (bias, std (D,H,W) float32: the mean of the samples, NaN where there is none, and their standard deviation,
    NaN where there are fewer than two; isummary (L, 3 + 4) int64: SURFACE_INT_COLUMNS, then per level q the voxels with at
    least two samples and |bias| <= z_q std, z_q = Phi^-1((1 + q) / 2); fsummary (L, 6) float64: SURFACE_FLOAT_COLUMNS), per
    label over the voxels of its fixed contour inside the mask, on the device.  No host synchronisation."""
    if seg_fixed.dim() != 5 or tuple(seg_fixed.shape[:2]) != (1, 1):
        raise L.IrsError(f'fixed segmentation must have shape (1,1,D,H,W), got {tuple(seg_fixed.shape)}')
    D, H, W = seg_fixed.shape[2:]
    _surface_state(mean, m2, count, (D, H, W))
    mask = _volume_mask(mask, D, H, W)
    lab, n = _labels(labels)
    levels = [float(q) for q in levels]
    if len(levels) > L.IRS_SURFACE_MAX_LEVELS or not all(0.0 < q < 1.0 for q in levels) or any(b <= a for a, b in zip(levels, levels[1:])):
        raise L.IrsError(f'levels must be 0 to {L.IRS_SURFACE_MAX_LEVELS} strictly increasing values in (0,1), got {levels}')
    z = [statistics.NormalDist().inv_cdf(0.5 * (1.0 + q)) for q in levels]
    dev = seg_fixed.device
    ptrs = [L.dev_ptr(seg_fixed, torch.int16), lab, n, L.dev_ptr(mean), L.dev_ptr(m2), L.dev_ptr(count), L.dev_ptr(mask, torch.uint8, True)]
    ws, isummary, fsummary = _summary_buffers(L.IRS_SURFACE_WS_BYTES, (max(n, 1), L.IRS_SURFACE_SUMMARY_INTS),
                                              (max(n, 1), L.IRS_SURFACE_SUMMARY_FLOATS), dev)
    bias = torch.empty((D, H, W), device=dev, dtype=torch.float32)
    std = torch.empty((D, H, W), device=dev, dtype=torch.float32)
    _call('irs_surface_posterior_finalize', *ptrs, (C.c_double * max(len(z), 1))(*z), len(z), L.dev_ptr(bias), L.dev_ptr(std),
          L.dev_ptr(isummary), L.dev_ptr(fsummary), L.dev_ptr(ws), L.IRS_SURFACE_WS_BYTES, D, H, W)
    return bias, std, isummary, fsummary


def chain_moments_update(x, mean, m2, half, k):
    """Welford update of half `half` of every chain's split-R-hat moments with the sample x (absent in the reference).
    x (C,3,D,H,W) float32; mean / m2 (2,C,3,D,H,W) float32, updated in place; k = samples in that half after this one."""
    Cn, D, H, W = _dims5(x, 3)
    _check_state(('mean', mean, (2, Cn, 3, D, H, W), None), ('m2', m2, (2, Cn, 3, D, H, W), None))
    _call('irs_chain_moments_update', L.dev_ptr(x, torch.float32), Cn, D, H, W, int(half), int(k), L.dev_ptr(mean, torch.float32),
          L.dev_ptr(m2, torch.float32))


def _split_moments(mean, m2):
    """(C, D, H, W) of the per-half moments mean / m2 (2,C,3,D,H,W) of chain_moments_update"""
    if mean.dim() != 6 or mean.shape[0] != 2 or mean.shape[2] != 3 or tuple(m2.shape) != tuple(mean.shape):
        raise L.IrsError(f'mean / m2 must have shape (2,C,3,D,H,W), got {tuple(mean.shape)} / {tuple(m2.shape)}')
    return mean.shape[1], mean.shape[3], mean.shape[4], mean.shape[5]


def split_rhat(mean, m2, n, mask=None, thresholds=(1.01, 1.1)):
    """Split-R-hat (BDA3 section 11.4) from the per-half moments of chain_moments_update, n samples per half.
    mask (D,H,W) bool / uint8 or None.  -> (rhat (D,H,W) float32, summary (5,) float64 on the device: voxels in the mask,
    voxels above thresholds[0], above thresholds[1], max, sum).  No host synchronisation."""
    Cn, D, H, W = _split_moments(mean, m2)
    mask = _volume_mask(mask, D, H, W)
    if len(thresholds) != 2:
        raise L.IrsError('split_rhat takes two thresholds')
    dev = mean.device
    ws, nbytes = _workspace('irs_split_rhat_workspace', Cn, D, H, W, device=dev)
    rhat = torch.empty((D, H, W), device=dev, dtype=torch.float32)
    summary = torch.empty(5, device=dev, dtype=torch.float64)
    _call('irs_split_rhat', L.dev_ptr(mean, torch.float32), L.dev_ptr(m2, torch.float32), Cn, int(n),
          L.dev_ptr(mask, torch.uint8, True), float(thresholds[0]), float(thresholds[1]), L.dev_ptr(rhat), L.dev_ptr(summary),
          L.dev_ptr(ws), nbytes, D, H, W)
    return rhat, summary


def chain_variogram_update(x, ring, vsum, k):
    """Online variogram of every chain's split sequences for the split ESS (absent in the reference; BDA3 section 11.5).
    x (C,3,D,H,W) float32; ring (L,C,3,D,H,W) and vsum (L,3,D,H,W) float32, updated in place; k = position in the current
    half after x (as for chain_moments_update): vsum[t-1] += sum over chains of (x - x_{-t})^2 for t <= min(k-1, L)."""
    Cn, D, H, W = _dims5(x, 3)
    if ring.dim() != 6 or tuple(ring.shape[1:]) != (Cn, 3, D, H, W):
        raise L.IrsError(f'ring must have shape (L,{Cn},3,{D},{H},{W}), got {tuple(ring.shape)}')
    Lg = ring.shape[0]
    _check_state(('vsum', vsum, (Lg, 3, D, H, W), None))
    _call('irs_chain_variogram_update', L.dev_ptr(x, torch.float32), Cn, D, H, W, int(k), Lg, L.dev_ptr(ring, torch.float32),
          L.dev_ptr(vsum, torch.float32))


def split_ess(mean, m2, vsum, n, mask=None, threshold=400.0):
    """Split ESS and MCSE of the posterior mean (BDA3 section 11.5) from the per-half moments of chain_moments_update and the
    lag sums of chain_variogram_update, n samples per half.  mask (D,H,W) bool / uint8 or None.
    -> (ess (D,H,W) float32: min over the components, mcse (D,H,W) float32: max over the components, summary (5,) float64
    on the device: voxels in the mask, voxels with ESS < threshold, voxels with a truncated component, min ESS, sum of ESS).
    No host synchronisation."""
    Cn, D, H, W = _split_moments(mean, m2)
    if vsum.dim() != 5 or tuple(vsum.shape[1:]) != (3, D, H, W):
        raise L.IrsError(f'vsum must have shape (L,3,{D},{H},{W}), got {tuple(vsum.shape)}')
    mask = _volume_mask(mask, D, H, W)
    dev = mean.device
    ws, nbytes = _workspace('irs_split_ess_workspace', Cn, D, H, W, device=dev)
    ess = torch.empty((D, H, W), device=dev, dtype=torch.float32)
    mcse = torch.empty((D, H, W), device=dev, dtype=torch.float32)
    summary = torch.empty(5, device=dev, dtype=torch.float64)
    _call('irs_split_ess', L.dev_ptr(mean, torch.float32), L.dev_ptr(m2, torch.float32), L.dev_ptr(vsum, torch.float32), Cn, int(n),
          vsum.shape[0], L.dev_ptr(mask, torch.uint8, True), float(threshold), L.dev_ptr(ess), L.dev_ptr(mcse), L.dev_ptr(summary),
          L.dev_ptr(ws), nbytes, D, H, W)
    return ess, mcse, summary


def label_posterior_update(seg_warped, labels, counts, volume, records_before):
    """Fold one recorded step into the posterior label maps (absent in the reference): seg_warped (C,1,D,H,W) int16, every
    chain's nearest-neighbour warp of the moving segmentation; labels: the K label values; counts (K,D,H,W) int32 += 1 where
    a map carries the structure; volume (K,2) float64 {mean, M2} of the per-record volumes, Welford-folded in chain order
    after `records_before` records.  No host synchronisation."""
    if seg_warped.dim() != 5 or seg_warped.shape[1] != 1:
        raise L.IrsError(f'seg_warped must have shape (C,1,D,H,W), got {tuple(seg_warped.shape)}')
    Cn, D, H, W = seg_warped.shape[0], *seg_warped.shape[2:]
    lab, K = _labels(labels)
    if tuple(counts.shape) != (K, D, H, W) or counts.dtype != torch.int32:
        raise L.IrsError(f'counts must be a ({K},{D},{H},{W}) int32 tensor, got {counts.dtype} {tuple(counts.shape)}')
    if tuple(volume.shape) != (K, 2) or volume.dtype != torch.float64:
        raise L.IrsError(f'volume must be a ({K},2) float64 tensor, got {volume.dtype} {tuple(volume.shape)}')
    ws, nbytes = _workspace('irs_label_posterior_workspace', Cn, K, D, H, W, device=seg_warped.device)
    _call('irs_label_posterior_update', L.dev_ptr(seg_warped, torch.int16), Cn, D, H, W, lab, K, L.dev_ptr(counts, torch.int32),
          L.dev_ptr(volume, torch.float64), int(records_before), L.dev_ptr(ws), nbytes)


def label_posterior_finalize(counts, n, labels, seg_fixed, mask=None):
    """Entropy and MAP maps and the whole-volume sums of the posterior label maps after n records (absent in the reference).
    counts (K,D,H,W) int32; seg_fixed (D,H,W) int16 (a leading (1,1) is accepted); mask (D,H,W) bool / uint8 or None.
    -> (entropy (D,H,W) float32, map_label (D,H,W) int16, summary (K, 6 + 3 * IRS_LABEL_BINS) int64, mask_summary (4,)
    float64), all on the device: include/irsgmcmc.h gives the columns.  No host synchronisation."""
    if counts.dim() != 4:
        raise L.IrsError(f'counts must have shape (K,D,H,W), got {tuple(counts.shape)}')
    K, D, H, W = counts.shape
    lab, nl = _labels(labels)
    if nl != K:
        raise L.IrsError(f'{nl} labels for {K} count planes')
    if seg_fixed.numel() != D * H * W or seg_fixed.shape[-3:] != (D, H, W):
        raise L.IrsError(f'seg_fixed must be a ({D},{H},{W}) volume, got {tuple(seg_fixed.shape)}')
    seg_fixed = seg_fixed.reshape(D, H, W).contiguous()
    mask = _volume_mask(mask, D, H, W)
    dev = counts.device
    ws, nbytes = _workspace('irs_label_posterior_workspace', 1, K, D, H, W, device=dev)
    entropy = torch.empty((D, H, W), device=dev, dtype=torch.float32)
    map_label = torch.empty((D, H, W), device=dev, dtype=torch.int16)
    summary = torch.empty((K, 6 + 3 * L.IRS_LABEL_BINS), device=dev, dtype=torch.int64)
    mask_summary = torch.empty(4, device=dev, dtype=torch.float64)
    _call('irs_label_posterior_finalize', L.dev_ptr(counts, torch.int32), K, D, H, W, int(n), lab, L.dev_ptr(seg_fixed, torch.int16),
          L.dev_ptr(mask, torch.uint8, True), L.dev_ptr(entropy), L.dev_ptr(map_label), L.dev_ptr(summary), L.dev_ptr(mask_summary),
          L.dev_ptr(ws), nbytes)
    return entropy, map_label, summary, mask_summary


def _jacobian_state(folds, mean, m2, shape):
    _check_state(('folds', folds, shape, torch.int32), ('mean', mean, shape, torch.float32), ('m2', m2, shape, torch.float32))


def jacobian_posterior_update(transformation, folds, mean, m2, records_before):
    """Fold one recorded step into the Jacobian posterior (absent in the reference, which keeps one fold count per sample:
    utils/util.py:209-212): transformation (C,3,D,H,W) float32 in normalised coordinates, every chain's sample; folds (D,H,W)
    int32 += 1 where a record's det J is not > 0; mean / m2 (D,H,W) float32: Welford moments of log det J over the other
    records, folded in chain order after `records_before` records.  No host synchronisation."""
    Cn, D, H, W = _dims5(transformation, 3)
    _jacobian_state(folds, mean, m2, (D, H, W))
    _call('irs_jacobian_posterior_update', L.dev_ptr(transformation, torch.float32), Cn, D, H, W, L.dev_ptr(folds, torch.int32),
          L.dev_ptr(mean, torch.float32), L.dev_ptr(m2, torch.float32), int(records_before))


def jacobian_posterior_finalize(folds, mean, m2, n, mask=None):
    """The maps and the masked summary of the Jacobian posterior after n records (absent in the reference).  folds (D,H,W)
    int32, mean / m2 (D,H,W) float32; mask (D,H,W) bool / uint8 or None.  -> (fold_prob, logJ_mean, logJ_std, all (D,H,W)
    float32, isummary (4,) int64, fsummary (5,) float64), all on the device: include/irsgmcmc.h gives the columns.
    No host synchronisation."""
    if folds.dim() != 3:
        raise L.IrsError(f'folds must have shape (D,H,W), got {tuple(folds.shape)}')
    D, H, W = folds.shape
    _jacobian_state(folds, mean, m2, (D, H, W))
    mask = _volume_mask(mask, D, H, W)
    dev = folds.device
    ws, isummary, fsummary = _summary_buffers(L.IRS_JACOBIAN_WS_BYTES, L.IRS_JACOBIAN_SUMMARY_INTS, L.IRS_JACOBIAN_SUMMARY_FLOATS, dev)
    fold_prob, logj_mean, logj_std = (torch.empty((D, H, W), device=dev, dtype=torch.float32) for _ in range(3))
    _call('irs_jacobian_posterior_finalize', L.dev_ptr(folds, torch.int32), L.dev_ptr(mean, torch.float32),
          L.dev_ptr(m2, torch.float32), D, H, W, int(n), L.dev_ptr(mask, torch.uint8, True), L.dev_ptr(fold_prob),
          L.dev_ptr(logj_mean), L.dev_ptr(logj_std), L.dev_ptr(isummary), L.dev_ptr(fsummary), L.dev_ptr(ws),
          L.IRS_JACOBIAN_WS_BYTES)
    return fold_prob, logj_mean, logj_std, isummary, fsummary


def _covariance_state(mean, comoment, shape):
    _check_state(('mean', mean, (3, *shape), torch.float32), ('comoment', comoment, (6, *shape), torch.float32))


def displacement_covariance_update(displacement, mean, comoment, records_before):
    """Fold one recorded step into the displacement covariance posterior (absent in the reference, which keeps three
    per-component standard deviations): displacement (C,3,D,H,W) float32 in normalised coordinates, every chain's sample; mean
    (3,D,H,W) and comoment (6,D,H,W: xx, yy, zz, xy, xz, yz) float32: the Welford moments, folded in chain order after
    `records_before` records (0 overwrites the state).  No host synchronisation."""
    Cn, D, H, W = _dims5(displacement, 3)
    _covariance_state(mean, comoment, (D, H, W))
    _call('irs_displacement_covariance_update', L.dev_ptr(displacement, torch.float32), Cn, D, H, W, L.dev_ptr(mean, torch.float32),
          L.dev_ptr(comoment, torch.float32), int(records_before))


def displacement_covariance_finalize(mean, comoment, n, scale, mask=None):
    """The maps and the masked summary of the displacement covariance posterior after n records (absent in the reference).
    mean (3,D,H,W), comoment (6,D,H,W) float32; scale: three positive floats, one per channel; mask (D,H,W) bool / uint8 or
    None.  -> (std (3,D,H,W), direction (3,D,H,W), anisotropy (D,H,W), all float32, isummary (2,) int64, fsummary (8,)
    float64), all on the device: include/irsgmcmc.h gives the columns.  No host synchronisation."""
    if mean.dim() != 4:
        raise L.IrsError(f'mean must have shape (3,D,H,W), got {tuple(mean.shape)}')
    D, H, W = mean.shape[1:]
    _covariance_state(mean, comoment, (D, H, W))
    mask = _volume_mask(mask, D, H, W)
    scale = _three_floats(scale, lambda v: f'scale must hold three floats, got {len(v)}')
    dev = mean.device
    ws, isummary, fsummary = _summary_buffers(L.IRS_COVARIANCE_WS_BYTES, L.IRS_COVARIANCE_SUMMARY_INTS, L.IRS_COVARIANCE_SUMMARY_FLOATS,
                                              dev)
    std, direction = (torch.empty((3, D, H, W), device=dev, dtype=torch.float32) for _ in range(2))
    anisotropy = torch.empty((D, H, W), device=dev, dtype=torch.float32)
    _call('irs_displacement_covariance_finalize', L.dev_ptr(mean, torch.float32), L.dev_ptr(comoment, torch.float32), D, H, W, int(n),
          scale, L.dev_ptr(mask, torch.uint8, True), L.dev_ptr(std), L.dev_ptr(direction), L.dev_ptr(anisotropy),
          L.dev_ptr(isummary), L.dev_ptr(fsummary), L.dev_ptr(ws), L.IRS_COVARIANCE_WS_BYTES)
    return std, direction, anisotropy, isummary, fsummary


def _quantile_state(centre, hist, shape):
    """the number of bins of hist (3,bins,D,H,W), its second extent"""
    bins = int(hist.shape[1] if hist.dim() == 5 else 0)
    if not (L.IRS_QUANTILE_MIN_BINS <= bins <= L.IRS_QUANTILE_MAX_BINS) or bins % 2:
        raise L.IrsError(f'bins must be an even number in {L.IRS_QUANTILE_MIN_BINS}..{L.IRS_QUANTILE_MAX_BINS}, got {bins}')
    _check_state(('centre', centre, (3, *shape), torch.float32), ('hist', hist, (3, bins, *shape), torch.uint16))
    return bins


def displacement_quantiles_update(displacement, centre, hist, inv_width, records_before):
    """Count one recorded step into the displacement histograms behind the credible intervals (absent in the reference, which
    keeps moments only): displacement (C,3,D,H,W) float32 in normalised coordinates, every chain's sample; centre (3,D,H,W)
    float32 and hist (3,bins,D,H,W) uint16, bin-major; inv_width: three positive floats, one per channel (rounded to float32).
    `records_before` records were counted before: 0 writes centre from chain 0 and overwrites hist; records_before + C may
    not exceed IRS_QUANTILE_MAX_RECORDS, what a uint16 count holds.  include/irsgmcmc.h gives the bin of a value.  No host
    synchronisation."""
    Cn, D, H, W = _dims5(displacement, 3)
    bins = _quantile_state(centre, hist, (D, H, W))
    records_before = int(records_before)
    if records_before < 0 or records_before + Cn > L.IRS_QUANTILE_MAX_RECORDS:
        raise L.IrsError(f'{records_before} + {Cn} records: a uint16 count holds 0..{L.IRS_QUANTILE_MAX_RECORDS}')
    _call('irs_displacement_quantiles_update', L.dev_ptr(displacement, torch.float32), Cn, D, H, W, L.dev_ptr(centre, torch.float32),
          L.dev_ptr(hist, torch.uint16), bins, _three_positive('inv_width', inv_width), records_before)


def displacement_quantiles_finalize(centre, hist, n, width, scale, probs, mask=None):
    """The quantile maps, the width of the credible band and its masked summary after n records (absent in the reference).
    centre (3,D,H,W) float32, hist (3,bins,D,H,W) uint16; width, scale: three positive floats each, one per channel; probs:
    2..IRS_QUANTILE_MAX_PROBS strictly increasing probabilities in (0,1); mask (D,H,W) bool / uint8 or None.  -> (quantiles
    (P,3,D,H,W), ci_width (D,H,W), float32, isummary (3,) int64, fsummary (5,) float64), all on the device:
    include/irsgmcmc.h gives the definitions and the columns.  No host synchronisation."""
    if centre.dim() != 4:
        raise L.IrsError(f'centre must have shape (3,D,H,W), got {tuple(centre.shape)}')
    D, H, W = centre.shape[1:]
    bins = _quantile_state(centre, hist, (D, H, W))
    mask = _volume_mask(mask, D, H, W)
    probs = [float(p) for p in probs]
    if not 2 <= len(probs) <= L.IRS_QUANTILE_MAX_PROBS:
        raise L.IrsError(f'probs must hold 2..{L.IRS_QUANTILE_MAX_PROBS} probabilities, got {len(probs)}')
    if not all(0.0 < p < 1.0 for p in probs) or any(b <= a for a, b in zip(probs, probs[1:])):
        raise L.IrsError(f'probs must be strictly increasing in (0,1), got {probs}')
    n = int(n)
    if not 1 <= n <= L.IRS_QUANTILE_MAX_RECORDS:
        raise L.IrsError(f'n = {n} records, 1..{L.IRS_QUANTILE_MAX_RECORDS} needed')
    width, scale = _three_positive('width', width), _three_positive('scale', scale)
    dev, P = centre.device, len(probs)
    ws, isummary, fsummary = _summary_buffers(L.IRS_QUANTILE_WS_BYTES, L.IRS_QUANTILE_SUMMARY_INTS, L.IRS_QUANTILE_SUMMARY_FLOATS, dev)
    quantiles = torch.empty((P, 3, D, H, W), device=dev, dtype=torch.float32)
    ci_width = torch.empty((D, H, W), device=dev, dtype=torch.float32)
    _call('irs_displacement_quantiles_finalize', L.dev_ptr(centre, torch.float32), L.dev_ptr(hist, torch.uint16), bins, D, H, W, n,
          width, scale, (C.c_double * P)(*probs), P, L.dev_ptr(mask, torch.uint8, True), L.dev_ptr(quantiles), L.dev_ptr(ci_width),
          L.dev_ptr(isummary), L.dev_ptr(fsummary), L.dev_ptr(ws), L.IRS_QUANTILE_WS_BYTES)
    return quantiles, ci_width, isummary, fsummary


def svf_exp_inverse(v, no_steps=12):
    """The inverse of SVF_3D.forward's map: exp(-v) by the same scaling and squaring (absent in the reference, which only
    evaluates the forward map).  v (C,3,D,H,W) float32 in voxel units.  -> (transformation in [-1,1] coordinates, displacement
    in voxels), bit-identical to svf_exp_fwd(-v); the workspace is two fields, nothing is kept for a backward.  No host
    synchronisation."""
    Cn, D, H, W = _dims5(v, 3)
    scratch = torch.empty((2,) + tuple(v.shape), device=v.device, dtype=torch.float32)
    t, d = torch.empty_like(v), torch.empty_like(v)
    _call('irs_svf_exp_inverse', L.dev_ptr(v, torch.float32), L.dev_ptr(scratch), L.dev_ptr(t), L.dev_ptr(d), int(no_steps), Cn, D, H, W)
    return t, d


def inverse_consistency(t_a, d_a, d_b, scale=None, mask=None, want_residual=False):
    """Inverse-consistency error of a pair of maps (absent in the reference): per chain and voxel r = d_a(x) +
    trilinear(d_b)(t_a(x)).  t_a (C,3,D,H,W) float32: a transformation in [-1,1] coordinates; d_a, d_b (C,3,D,H,W) float32:
    displacements in one common unit; scale: three positive floats, one per channel (default 1: the unit of the
    displacements); mask: bool / uint8, (1 or C,1,D,H,W) or (D,H,W), or None.  -> (norm (C,1,D,H,W) float32 =
    sqrt(sum_c (scale_c r_c)^2), residual (C,3,D,H,W) float32 or None, isummary (C,2) int64, fsummary (C,3) float64), all on
    the device: include/irsgmcmc.h gives the columns.  (t, d, d_inv) gives phi^-1 o phi - id on the fixed grid, (t_inv, d_inv,
    d) gives phi o phi^-1 - id on the moving grid.  No host synchronisation."""
    Cn, D, H, W = _dims5(t_a, 3)
    for name, t in (('d_a', d_a), ('d_b', d_b)):
        if tuple(t.shape) != tuple(t_a.shape):
            raise L.IrsError(f'{name} shape {tuple(t.shape)} does not match t_a {tuple(t_a.shape)}')
    mask_chains = 1
    if mask is not None:
        if mask.dtype not in (torch.bool, torch.uint8) or mask.numel() not in (D * H * W, Cn * D * H * W) or \
                tuple(mask.shape[-3:]) != (D, H, W):
            raise L.IrsError(f'mask must be a bool / uint8 (1 or {Cn},1,{D},{H},{W}) tensor, got {mask.dtype} {tuple(mask.shape)}')
        mask_chains = mask.numel() // (D * H * W)
        mask = _as_uint8(mask)
    dev = t_a.device
    ws, isummary, fsummary = _summary_buffers(L.IRS_ICE_WS_BYTES, (Cn, L.IRS_ICE_SUMMARY_INTS), (Cn, L.IRS_ICE_SUMMARY_FLOATS), dev)
    norm = torch.empty((Cn, 1, D, H, W), device=dev, dtype=torch.float32)
    residual = torch.empty_like(t_a) if want_residual else None
    _call('irs_inverse_consistency', L.dev_ptr(t_a, torch.float32), L.dev_ptr(d_a, torch.float32), L.dev_ptr(d_b, torch.float32),
          _three_positive('scale', (1.0, 1.0, 1.0) if scale is None else scale), L.dev_ptr(mask, torch.uint8, True), mask_chains,
          L.dev_ptr(residual, None, True), L.dev_ptr(norm), L.dev_ptr(isummary), L.dev_ptr(fsummary), L.dev_ptr(ws),
          L.IRS_ICE_WS_BYTES, Cn, D, H, W)
    return norm, residual, isummary, fsummary


def _ice_state(mean, peak, shape):
    _check_state(('mean', mean, shape, torch.float32), ('peak', peak, shape, torch.float32))


def inverse_consistency_update(norm, mean, peak, records_before):
    """Fold one recorded step of inverse-consistency norm maps into their per-voxel posterior (absent in the reference): norm
    (C,1,D,H,W) float32, every chain's map; mean / peak (D,H,W) float32: the Welford mean and the running maximum of the
    finite values, folded in chain order after `records_before` records (0 overwrites the state).  Non-finite values
    propagate into mean; peak is NaN where no value was ever finite.  No host synchronisation."""
    Cn, D, H, W = _dims5(norm, 1)
    _ice_state(mean, peak, (D, H, W))
    _call('irs_inverse_consistency_update', L.dev_ptr(norm, torch.float32), Cn, D, H, W, L.dev_ptr(mean, torch.float32),
          L.dev_ptr(peak, torch.float32), int(records_before))


def inverse_consistency_finalize(mean, peak, threshold, mask=None):
    """The masked summary of the mean and peak inverse-consistency maps (absent in the reference).  mean / peak (D,H,W)
    float32; threshold: a finite float > 0 in the unit of the maps; mask (D,H,W) bool / uint8 or None.  -> (isummary (3,) int64
    {voxels, voxels with a non-finite mean, voxels with peak > threshold}, fsummary (3,) float64 {sum mean, max mean, max
    peak}), on the device.  No host synchronisation."""
    if mean.dim() != 3:
        raise L.IrsError(f'mean must have shape (D,H,W), got {tuple(mean.shape)}')
    D, H, W = mean.shape
    _ice_state(mean, peak, (D, H, W))
    mask = _volume_mask(mask, D, H, W)
    threshold = float(threshold)
    if not (math.isfinite(threshold) and threshold > 0):
        raise L.IrsError(f'threshold must be a finite float > 0, got {threshold}')
    ws, isummary, fsummary = _summary_buffers(L.IRS_ICE_MAP_WS_BYTES, L.IRS_ICE_MAP_SUMMARY_INTS, L.IRS_ICE_MAP_SUMMARY_FLOATS,
                                              mean.device)
    _call('irs_inverse_consistency_finalize', L.dev_ptr(mean, torch.float32), L.dev_ptr(peak, torch.float32), D, H, W,
          L.dev_ptr(mask, torch.uint8, True), threshold, L.dev_ptr(isummary), L.dev_ptr(fsummary), L.dev_ptr(ws),
          L.IRS_ICE_MAP_WS_BYTES)
    return isummary, fsummary


def native_warp(displacement, grid, im=None, seg=None, mask=None, fill=None, want_displacement=None):
    """A sampled transformation applied on the image's own voxel grid (absent in the reference, whose outputs all live on the
    registration grid).  displacement (C,3,*grid.dims) float32 in [-1,1] coordinates; grid: a native.NativeGrid; im float32 /
    seg int16 / mask bool or uint8: the UNPADDED native moving volumes, (1 or C,1,*grid.shape) with one leading size for all of
    them, or None; fill: what the data set padded the image with (its minimum; default: the minimum of `im`, one host
    read-back); want_displacement: None, or the three per-channel factors of the displacement output (grid.voxel_scale() for
    native voxels, grid.mm_scale() for mm).  -> a dict with 'im' (C,1,*shape) float32 (trilinear), 'seg' int16 / 'mask' (nearest)
    and 'displacement' (C,3,*shape) float32, each present when asked for: grid_sample (border, align_corners) of the padded
    native volume at identity + the displacement resized to the padded extent, cropped to the native box, in ONE launch that
    forms neither the padded volumes nor the resized field (include/irsgmcmc.h: irs_native_warp).  No host synchronisation
    when `fill` is given."""
    Cn, D, H, W = _dims5(displacement, 3)
    if (D, H, W) != tuple(grid.dims):
        raise L.IrsError(f'displacement {tuple(displacement.shape)} is not on the registration grid {tuple(grid.dims)}')
    n = tuple(grid.shape)
    given = [(k, t) for k, t in (('im', im), ('seg', seg), ('mask', mask)) if t is not None]
    if not given and want_displacement is None:
        raise L.IrsError('native_warp: nothing asked for (im, seg, mask and want_displacement are all None)')
    dtypes = {'im': (torch.float32,), 'seg': (torch.int16,), 'mask': (torch.bool, torch.uint8)}
    for k, t in given:
        _chain_volumes(k, t, 'the native grid', Cn, *n)
        if t.dtype not in dtypes[k]:
            raise L.IrsError(f'{k} must be {" / ".join(str(d) for d in dtypes[k])}, got {t.dtype}')
        if t.shape[0] != given[0][1].shape[0]:
            raise L.IrsError(f'the moving volumes must share their leading size: {given[0][0]} has {given[0][1].shape[0]}, '
                             f'{k} has {t.shape[0]}')
    if im is not None and fill is None:
        fill = float(im.min())
    fill = 0.0 if fill is None else float(fill)
    if not math.isfinite(fill):
        raise L.IrsError(f'fill must be finite, got {fill}')
    scale = None
    if want_displacement is not None:
        scale = _three_floats(want_displacement, lambda v: f'want_displacement must hold three finite floats, got {v}', math.isfinite)
    dev = displacement.device
    out = {}
    if im is not None:
        out['im'] = torch.empty((Cn, 1, *n), device=dev, dtype=torch.float32)
    if seg is not None:
        out['seg'] = torch.empty((Cn, 1, *n), device=dev, dtype=torch.int16)
    if mask is not None:
        out['mask'] = torch.empty((Cn, 1, *n), device=dev, dtype=mask.dtype)
    if scale is not None:
        out['displacement'] = torch.empty((Cn, 3, *n), device=dev, dtype=torch.float32)
    i3 = lambda v: (C.c_int32 * 3)(*[int(x) for x in v])
    _call('irs_native_warp', L.dev_ptr(displacement, torch.float32), Cn, i3(grid.dims), i3(n), i3(grid.padding),
          L.dev_ptr(im, None, True), L.dev_ptr(seg, None, True), L.dev_ptr(mask, None, True), given[0][1].shape[0] if given else 1,
          fill, scale, L.dev_ptr(out.get('im'), None, True), L.dev_ptr(out.get('seg'), None, True),
          L.dev_ptr(out.get('mask'), None, True), L.dev_ptr(out.get('displacement'), None, True))
    return out


SIMILARITY_COLUMNS = ('n', 'n_nonfinite', 'n_clipped', 'mse', 'ncc', 'h_fixed', 'h_moving', 'h_joint', 'mi', 'nmi')


def intensity_ranges(*images):
    """(lo, hi) of the finite values of every image, as Python floats: ONE host read-back for all of them"""
    ext = []
    for im in images:
        finite = torch.isfinite(im)
        ext += [torch.where(finite, im, math.inf).min(), torch.where(finite, im, -math.inf).max()]
    ext = torch.stack(ext).tolist()
    return [(ext[2 * i], ext[2 * i + 1]) for i in range(len(images))]


def _ranges(fixed, fixed_range, moving, moving_range):
    """the two (lo, hi): a None becomes that image's intensity_ranges, with one host read-back for both and none when both are
    given"""
    missing = [im for im, r in ((fixed, fixed_range), (moving, moving_range)) if r is None]
    found = iter(intensity_ranges(*missing)) if missing else None
    return [r if r is not None else next(found) for r in (fixed_range, moving_range)]


def image_similarity(fixed, moving, mask=None, bins=64, fixed_range=None, moving_range=None, want_hist=False):
    """Intensity similarity of the fixed image and a (warped) moving image (absent in the reference): fixed (1 or C,1,D,H,W) and
    moving (C,1,D,H,W) float32; mask (1,1,D,H,W) bool / uint8 shared by the chains, or None; bins in 2 .. 128; fixed_range /
    moving_range: (lo, hi), finite with hi > lo -- None: the min / max of the finite values of that image (one host read-back;
    with both ranges given the call does not synchronise).  -> {'stats': (C,10) float64 on the device, columns
    SIMILARITY_COLUMNS[, 'hist': (C,bins,bins) int32, hist[c][bin of fixed][bin of moving]]}: the joint histogram and the
    moment sums from ONE pass over the two volumes, then entropies, MI, NMI, MSE and the global NCC per chain
    (include/irsgmcmc.h: irs_image_similarity)."""
    Cn, D, H, W = _dims5(moving, 1)
    _chain_volumes('fixed', fixed, 'moving', Cn, D, H, W)
    mask = _shared_mask(mask, D, H, W)
    if isinstance(bins, bool) or not isinstance(bins, int):
        raise L.IrsError(f'bins must be an integer, got {bins!r}')
    fixed_ptr, moving_ptr = L.dev_ptr(fixed, torch.float32), L.dev_ptr(moving, torch.float32)
    fixed_range, moving_range = _ranges(fixed, fixed_range, moving, moving_range)
    f_lo, f_hi = (float(x) for x in fixed_range)
    m_lo, m_hi = (float(x) for x in moving_range)
    dev = moving.device
    ws, nbytes = _workspace('irs_image_similarity_workspace', Cn, bins, device=dev)
    out = {'stats': torch.empty((Cn, L.IRS_SIMILARITY_STATS), device=dev, dtype=torch.float64)}
    if want_hist:
        out['hist'] = torch.empty((Cn, bins, bins), device=dev, dtype=torch.int32)
    _call('irs_image_similarity', fixed_ptr, fixed.shape[0], moving_ptr, Cn, L.dev_ptr(mask, torch.uint8, True), D, H, W, f_lo, f_hi,
          m_lo, m_hi, bins, L.dev_ptr(out.get('hist'), None, True), L.dev_ptr(out['stats']), L.dev_ptr(ws), nbytes)
    return out


LOCAL_COLUMNS = ('n', 'n_flat', 'n_nonfinite', 'lncc_mean', 'lncc_min', 'ssim_mean', 'ssim_min')
LOCAL_MAPS = ('lncc', 'ssim')


def local_similarity_constants(fixed_range, moving_range):
    """(floor_f, floor_m, c1, c2) of local_similarity from the two intensity ranges (lo, hi): a window is flat when its variance
    is not above floor_x = (1e-3 (hi - lo))^2; with L = max(f_hi, m_hi) - min(f_lo, m_lo) the SSIM constants are c1 = (0.01 L)^2
    and c2 = (0.03 L)^2.  Python floats (float64); both ranges finite with hi > lo."""
    (f_lo, f_hi), (m_lo, m_hi) = ((float(x) for x in r) for r in (fixed_range, moving_range))
    for name, lo, hi in (('fixed', f_lo, f_hi), ('moving', m_lo, m_hi)):
        if not (math.isfinite(lo) and math.isfinite(hi) and hi > lo):
            raise L.IrsError(f'{name} range [{lo}, {hi}]: finite bounds with hi > lo needed')
    span = max(f_hi, m_hi) - min(f_lo, m_lo)
    return (1e-3 * (f_hi - f_lo)) ** 2, (1e-3 * (m_hi - m_lo)) ** 2, (0.01 * span) ** 2, (0.03 * span) ** 2


def local_similarity(fixed, moving, mask=None, radius=2, fixed_range=None, moving_range=None, want=LOCAL_MAPS):
    """Where two images agree (absent in the reference): the local normalised cross-correlation and SSIM of every voxel's
    (2 radius + 1)^3 box window with clamped indices.  fixed (1 or C,1,D,H,W) and moving (C,1,D,H,W) float32; mask (1,1,D,H,W)
    bool / uint8 shared by the chains, or None: it selects the voxels of the statistics, never those of a window; radius in
    1 .. 4; fixed_range / moving_range: (lo, hi), finite with hi > lo -- None: the min / max of the finite values of that image
    (one host read-back; with both given the call does not synchronise) -- which give the flatness floors and the SSIM
    constants (local_similarity_constants); want: which of 'lncc', 'ssim' to write.  -> {'stats': (C,7) float64 on the device,
    columns LOCAL_COLUMNS[, 'lncc': (C,1,D,H,W) float32][, 'ssim': ...]}; LNCC is NaN where a window is flat, both maps where
    it holds a non-finite value (include/irsgmcmc.h: irs_local_similarity)."""
    Cn, D, H, W = _dims5(moving, 1)
    _chain_volumes('fixed', fixed, 'moving', Cn, D, H, W)
    mask = _shared_mask(mask, D, H, W)
    if isinstance(radius, bool) or not isinstance(radius, int):
        raise L.IrsError(f'radius must be an integer, got {radius!r}')
    want = tuple(want)
    if any(w not in LOCAL_MAPS for w in want):
        raise L.IrsError(f'want must list names out of {LOCAL_MAPS}, got {want}')
    fixed_ptr, moving_ptr = L.dev_ptr(fixed, torch.float32), L.dev_ptr(moving, torch.float32)
    consts = local_similarity_constants(*_ranges(fixed, fixed_range, moving, moving_range))
    dev = moving.device
    ws = torch.empty(L.IRS_LOCAL_WS_BYTES, device=dev, dtype=torch.uint8)
    out = {'stats': torch.empty((Cn, L.IRS_LOCAL_STATS), device=dev, dtype=torch.float64)}
    for name in LOCAL_MAPS:
        if name in want:
            out[name] = torch.empty((Cn, 1, D, H, W), device=dev, dtype=torch.float32)
    _call('irs_local_similarity', fixed_ptr, fixed.shape[0], moving_ptr, Cn, L.dev_ptr(mask, torch.uint8, True), D, H, W, radius,
          *consts, L.dev_ptr(out.get('lncc'), None, True), L.dev_ptr(out.get('ssim'), None, True), L.dev_ptr(out['stats']),
          L.dev_ptr(ws), L.IRS_LOCAL_WS_BYTES)
    return out


def _local_state(mean, low, count, shape):
    _check_state(('mean', mean, shape, torch.float32), ('low', low, shape, torch.float32), ('count', count, shape, torch.int32))


def local_similarity_update(lncc, mean, low, count, records_before):
    """Fold one recorded step of LNCC maps into their per-voxel posterior (absent in the reference): lncc (C,1,D,H,W) float32,
    every chain's map; mean / low (D,H,W) float32 and count (D,H,W) int32: the streaming mean, the minimum and the number of
    the samples that are no NaN, folded in chain order after `records_before` records (0 overwrites the state).  No host
    synchronisation."""
    Cn, D, H, W = _dims5(lncc, 1)
    _local_state(mean, low, count, (D, H, W))
    _call('irs_local_similarity_update', L.dev_ptr(lncc, torch.float32), Cn, D, H, W, L.dev_ptr(mean), L.dev_ptr(low),
          L.dev_ptr(count), int(records_before))


def local_similarity_finalize(mean, low, count, mask=None):
    """The masked summary of the LNCC posterior state (absent in the reference).  mean / low (D,H,W) float32, count (D,H,W)
    int32; mask (D,H,W) bool / uint8 or None.  -> (isummary (2,) int64 {voxels, voxels with count == 0}, fsummary (3,) float64
    {sum of mean, min of mean, min of low} over the voxels with count > 0), on the device.  No host synchronisation."""
    if mean.dim() != 3:
        raise L.IrsError(f'mean must have shape (D,H,W), got {tuple(mean.shape)}')
    D, H, W = mean.shape
    _local_state(mean, low, count, (D, H, W))
    mask = _volume_mask(mask, D, H, W)
    ws, isummary, fsummary = _summary_buffers(L.IRS_LOCAL_MAP_WS_BYTES, L.IRS_LOCAL_MAP_SUMMARY_INTS, L.IRS_LOCAL_MAP_SUMMARY_FLOATS,
                                              mean.device)
    _call('irs_local_similarity_finalize', L.dev_ptr(mean), L.dev_ptr(low), L.dev_ptr(count), L.dev_ptr(mask, torch.uint8, True), D, H,
          W, L.dev_ptr(isummary), L.dev_ptr(fsummary), L.dev_ptr(ws), L.IRS_LOCAL_MAP_WS_BYTES)
    return isummary, fsummary


LANDMARK_COLUMNS = ('count', 'tre_mean', 'tre_std', 'tre_max', 'tre_of_mean', 'std_major', 'std_middle', 'std_minor', 'mahalanobis2',
                    'pit')
LANDMARK_STATE = (('mean', 3, torch.float64), ('comoment', 6, torch.float64), ('tre_mean', None, torch.float64),
                  ('tre_m2', None, torch.float64), ('tre_max', None, torch.float64), ('count', None, torch.int32))


def _points(name, t, K=None):
    if t.dim() != 2 or t.shape[1] != 3 or t.dtype != torch.float32 or (K is not None and t.shape[0] != K):
        raise L.IrsError(f'{name} must be a ({"K" if K is None else K},3) torch.float32 tensor, got {t.dtype} {tuple(t.shape)}')
    if not 1 <= t.shape[0] <= L.IRS_LANDMARK_MAX_POINTS:
        raise L.IrsError(f'{name}: K = {t.shape[0]} points, 1..{L.IRS_LANDMARK_MAX_POINTS} needed')
    return t.shape[0]


def transform_points(points, displacement, scale=(1.0, 1.0, 1.0), offset=None, want_sampled=False):
    """A displacement evaluated at K positions that need not be voxel centres (absent in the reference, which has no point-set
    operator).  points (K,3) float32 in [-1,1] coordinates, component 0 = x (the last axis); displacement (C,3,D,H,W) float32
    in any linear unit; scale: three positive floats, one per channel; offset (K,3) float32 or None (= 0).  -> mapped (C,K,3)
    float32 = scale_c * sampled_c + offset_c, or (mapped, sampled) with want_sampled: sampled (C,K,3) is the field sampled
    trilinearly at the point (border clamp, align_corners: a point on a voxel centre returns the stored value bit for bit).
    With the point's position in the output unit as the offset, mapped is the mapped point: warped(x) = moving(x + d(x)), so
    a point of the fixed grid lands in the moving image; the displacement of svf_exp_inverse carries points of the moving
    space to the fixed one.  A point with a non-finite coordinate gives NaN rows.  include/irsgmcmc.h has the rounding
    order.  No host synchronisation."""
    Cn, D, H, W = _dims5(displacement, 3)
    K = _points('points', points)
    if offset is not None:
        _points('offset', offset, K)
    dev = displacement.device
    mapped = torch.empty((Cn, K, 3), device=dev, dtype=torch.float32)
    sampled = torch.empty((Cn, K, 3), device=dev, dtype=torch.float32) if want_sampled else None
    _call('irs_transform_points', L.dev_ptr(points, torch.float32), K, L.dev_ptr(displacement, torch.float32), Cn, D, H, W,
          _three_positive('scale', scale), L.dev_ptr(offset, torch.float32, True), L.dev_ptr(sampled, None, True), L.dev_ptr(mapped))
    return (mapped, sampled) if want_sampled else mapped


def landmark_state(K, device):
    """a fresh state of the landmark posterior: {'mean' (K,3), 'comoment' (K,6: xx, xy, xz, yy, yz, zz), 'tre_mean', 'tre_m2',
    'tre_max' (K) float64, 'count' (K) int32}, all zero"""
    return {name: torch.zeros((K,) if ch is None else (K, ch), device=device, dtype=dtype) for name, ch, dtype in LANDMARK_STATE}


def _landmark_state(state, K):
    _check_state(*((name, state[name], (K,) if ch is None else (K, ch), dtype) for name, ch, dtype in LANDMARK_STATE))
    return [L.dev_ptr(state[name], dtype) for name, _, dtype in LANDMARK_STATE]


def landmark_update(mapped, target, state, records_before):
    """Fold one recorded step into the landmark posterior (absent in the reference): mapped (C,K,3) float32, every chain's
    mapped landmarks; target (K,3) float32, the corresponding points in the same unit; state: the dict of landmark_state,
    updated in place in float64 with the finite samples in chain order after `records_before` records (0 overwrites the
    state).  A non-finite sample is skipped for that landmark and not counted.  No host synchronisation."""
    if mapped.dim() != 3 or mapped.shape[2] != 3 or mapped.dtype != torch.float32:
        raise L.IrsError(f'mapped must be a (C,K,3) torch.float32 tensor, got {mapped.dtype} {tuple(mapped.shape)}')
    Cn, K = mapped.shape[:2]
    _points('target', target, K)
    _call('irs_landmark_update', L.dev_ptr(mapped, torch.float32), L.dev_ptr(target, torch.float32), Cn, K,
          *_landmark_state(state, K), int(records_before))


def landmark_finalize(state, target):
    """The per-landmark table and the summary of the landmark posterior (absent in the reference).  state: the dict of
    landmark_state; target (K,3) float32.  -> (table (K,10) float64 with the columns LANDMARK_COLUMNS, isummary (3,) int64
    {landmarks, landmarks without a finite sample, landmarks with a finite pit}, fsummary (4,) float64 {sum / max
    tre_of_mean, sum tre_mean, max tre_max} over the others), on the device: include/irsgmcmc.h gives the definitions.  No
    host synchronisation."""
    K = _points('target', target)
    ptrs = _landmark_state(state, K)
    dev = target.device
    ws, isummary, fsummary = _summary_buffers(L.IRS_LANDMARK_WS_BYTES, L.IRS_LANDMARK_SUMMARY_INTS, L.IRS_LANDMARK_SUMMARY_FLOATS, dev)
    table = torch.empty((K, L.IRS_LANDMARK_COLUMNS), device=dev, dtype=torch.float64)
    _call('irs_landmark_finalize', *ptrs, L.dev_ptr(target, torch.float32), K, L.dev_ptr(table), L.dev_ptr(isummary),
          L.dev_ptr(fsummary), L.dev_ptr(ws), L.IRS_LANDMARK_WS_BYTES)
    return table, isummary, fsummary
