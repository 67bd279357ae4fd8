"""Refusals of the C ABI that happen before any HIP runtime call (host-only: runs without a GPU), and the switch table.

Every case calls an entry point through ctypes with one bad argument and compares irs_last_error() with the message written out
here.  Device pointers are a dummy non-null address -- the argument checks never dereference them; the host arrays the checks do
read (scale, spacing, labels, boxes, probs, percentiles, dims / native / padding) are real.  EVERY case must be refused: a call that
passed validation would go on to launch.  The messages are part of the interface (callers and tests match on them): run this file
with IRS_LIB pointing at an older build of the library to see that a change of the host layer left them alone.
"""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from ir_sgmcmc_amd import _lib as L
from ir_sgmcmc_amd.engine import EngineConfig, irs_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x1000  # "a device pointer"
MAXC = L.IRS_MAX_CHAINS
I32MAX = 2 ** 31 - 1
NAN, INF = float('nan'), float('inf')


def f3(*v):
    return (C.c_float * 3)(*v)


def i32(*v):
    return (C.c_int32 * len(v))(*v)


def f64(*v):
    return (C.c_double * len(v))(*v)


ONES = f3(1, 1, 1)
LABELS = i32(1, 2)
BOXES = i32(*([0, 0, 0, 3, 3, 3] * 4))  # C = 2 chains x 2 labels, each box the whole 4^3 volume
PCT = f64(50, 95)
PROBS = f64(0.05, 0.95)
DIMS = dict(D=4, H=4, W=4)
_SIZE = C.c_size_t()

# Arguments that would PASS validation, by entry point and in the order of its signature; a case replaces some of them.
GOOD = {
    'irs_warp_fwd': dict(im=P, Cim=1, d_last=P, unif=None, alpha=0.0, warped=P, C=2, **DIMS, seed=0, iteration=0, stream=None),
    'irs_warp_bwd': dict(im=P, Cim=1, d_last=P, unif=None, alpha=0.0, g_warped=P, g_d=P, C=2, **DIMS, seed=0, iteration=0, stream=None),
    'irs_warp_transformation': dict(im=P, Cim=1, transformation=P, warped=P, C=2, **DIMS, stream=None),
    'irs_warp_nearest_u8': dict(seg=P, Cim=1, transformation=P, out=P, C=2, **DIMS, stream=None),
    'irs_warp_nearest_i16': dict(seg=P, Cim=1, transformation=P, out=P, C=2, **DIMS, stream=None),
    'irs_lcc_map_fwd': dict(fhat=P, Cf=1, warped=P, z=P, sigma_m=P, s=1, C=2, **DIMS, stream=None),
    'irs_lcc_map_bwd': dict(fhat=P, Cf=1, z=P, sigma_m=P, g_z=P, g_warped=P, s=1, C=2, **DIMS, stream=None),
    'irs_reg_energy': dict(v=P, y_out=P, partials=P, C=2, **DIMS, stream=None),
    'irs_label_boxes': dict(seg_fixed=P, Cf=1, seg_moving=P, labels=LABELS, n_labels=2, boxes=P, C=2, **DIMS, stream=None),
    'irs_surface_distance_workspace': dict(boxes=BOXES, n_pairs=4, **DIMS, bytes=C.byref(_SIZE)),
    'irs_label_surface_distance': dict(seg_fixed=P, Cf=1, seg_moving=P, labels=LABELS, n_labels=2, spacing=ONES, boxes=BOXES,
                                       workspace=P, workspace_bytes=3328, counts=P, sums=P, C=2, **DIMS, stream=None),
    'irs_hausdorff_workspace': dict(boxes=BOXES, n_pairs=4, Q=2, **DIMS, bytes=C.byref(_SIZE)),
    'irs_label_hausdorff_distance': dict(seg_fixed=P, Cf=1, seg_moving=P, labels=LABELS, n_labels=2, spacing=ONES, boxes=BOXES,
                                         workspace=P, workspace_bytes=69632, percentiles=PCT, Q=2, counts=P, sums=P, hd=P, hd_pct=P,
                                         C=2, **DIMS, stream=None),
    'irs_split_rhat': dict(mean=P, m2=P, C=2, n=4, mask=None, thr0=1.0, thr1=1.1, rhat=P, summary=P, ws=P, ws_bytes=40, **DIMS,
                           stream=None),
    'irs_split_ess': dict(mean=P, m2=P, vsum=P, C=2, n=8, L=4, mask=None, threshold=1.0, ess=P, mcse=P, summary=P, ws=P, ws_bytes=40,
                          **DIMS, stream=None),
    'irs_label_posterior_workspace': dict(C=2, K=2, **DIMS, bytes=C.byref(_SIZE)),
    'irs_label_posterior_update': dict(seg=P, C=2, **DIMS, labels=LABELS, K=2, counts=P, volume=P, records_before=0, ws=P, ws_bytes=16,
                                       stream=None),
    'irs_label_posterior_finalize': dict(counts=P, K=2, **DIMS, n=1, labels=LABELS, seg_fixed=P, mask=None, entropy=P, map_label=P,
                                         summary=P, mask_summary=P, ws=P, ws_bytes=608, stream=None),
    'irs_jacobian_posterior_update': dict(transformation=P, C=2, **DIMS, folds=P, mean=P, m2=P, records_before=0, stream=None),
    'irs_jacobian_posterior_finalize': dict(folds=P, mean=P, m2=P, **DIMS, n=1, mask=None, fold_prob=P, logJ_mean=P, logJ_std=P,
                                            isummary=P, fsummary=P, ws=P, ws_bytes=L.IRS_JACOBIAN_WS_BYTES, stream=None),
    'irs_displacement_covariance_update': dict(displacement=P, C=2, **DIMS, mean=P, comoment=P, records_before=0, stream=None),
    'irs_displacement_covariance_finalize': dict(mean=P, comoment=P, **DIMS, n=1, scale=ONES, mask=None, stdev=P, direction=P,
                                                 anisotropy=P, isummary=P, fsummary=P, ws=P, ws_bytes=L.IRS_COVARIANCE_WS_BYTES,
                                                 stream=None),
    'irs_displacement_quantiles_update': dict(displacement=P, C=2, **DIMS, centre=P, hist=P, bins=8, inv_width=ONES, records_before=0,
                                              stream=None),
    'irs_displacement_quantiles_finalize': dict(centre=P, hist=P, bins=8, **DIMS, n=1, width=ONES, scale=ONES, probs=PROBS, P=2,
                                                mask=None, quantiles=P, ci_width=P, isummary=P, fsummary=P, ws=P,
                                                ws_bytes=L.IRS_QUANTILE_WS_BYTES, stream=None),
    'irs_inverse_consistency': dict(t_a=P, d_a=P, d_b=P, scale=ONES, mask=None, mask_chains=1, residual=P, norm=P, isummary=P,
                                    fsummary=P, ws=P, ws_bytes=L.IRS_ICE_WS_BYTES, C=2, **DIMS, stream=None),
    'irs_inverse_consistency_update': dict(norm=P, C=2, **DIMS, mean=P, peak=P, records_before=0, stream=None),
    'irs_inverse_consistency_finalize': dict(mean=P, peak=P, **DIMS, mask=None, threshold=1.0, isummary=P, fsummary=P, ws=P,
                                             ws_bytes=L.IRS_ICE_MAP_WS_BYTES, stream=None),
    'irs_native_warp': dict(displacement=P, C=2, dims=i32(4, 4, 4), native=i32(6, 6, 6), padding=i32(1, 1, 1), im=P, seg=P, mask=P,
                            Cim=1, fill=0.0, scale=ONES, im_out=P, seg_out=P, mask_out=P, displacement_out=P, stream=None),
    'irs_transform_points': dict(points=P, K=3, displacement=P, C=2, **DIMS, scale=ONES, offset=None, sampled=P, mapped=P, stream=None),
    'irs_landmark_update': dict(mapped=P, target=P, C=2, K=3, mean=P, comoment=P, tre_mean=P, tre_m2=P, tre_max=P, count=P,
                                records_before=0, stream=None),
    'irs_landmark_finalize': dict(mean=P, comoment=P, tre_mean=P, tre_m2=P, tre_max=P, count=P, target=P, K=3, out=P, isummary=P,
                                  fsummary=P, ws=P, ws_bytes=L.IRS_LANDMARK_WS_BYTES, stream=None),
    'irs_image_similarity_workspace': dict(C=2, bins=8, bytes=C.byref(_SIZE)),
    'irs_image_similarity': dict(fixed=P, Cf=1, moving=P, C=2, mask=None, **DIMS, f_lo=0.0, f_hi=1.0, m_lo=0.0, m_hi=1.0, bins=8, hist=None,
                                 stats=P, ws=P, ws_bytes=74240, stream=None),
}

CASES = []  # (case id, entry point, replaced arguments, expected message, exact match)


def case(cid, fn, expected, exact=True, **bad):
    assert bad and set(bad) <= set(GOOD[fn]), (cid, fn)
    CASES.append((f'{fn[4:]}-{cid}', fn, bad, expected if expected.startswith('irs_') else f'{fn}: {expected}', exact))


# ---- chains_ok: C = 0 and C = IRS_MAX_CHAINS + 1.  Where dims_ok sees the chain count first, C = 0 is its "bad arguments".
for fn, zero in [('irs_label_posterior_update', None), ('irs_jacobian_posterior_update', 'bad arguments'),
                 ('irs_displacement_covariance_update', 'bad arguments'), ('irs_displacement_quantiles_update', 'bad arguments'),
                 ('irs_inverse_consistency', 'bad arguments'), ('irs_inverse_consistency_update', 'bad arguments'),
                 ('irs_native_warp', None), ('irs_transform_points', None), ('irs_landmark_update', None),
                 ('irs_image_similarity_workspace', None), ('irs_image_similarity', None)]:
    case('C=0', fn, zero or f'C = 0 chains, 1..{MAXC}', C=0)
    case('C=max+1', fn, f'C = {MAXC + 1} chains, 1..{MAXC}', C=MAXC + 1)

# ---- chain_count_ok / broadcast_ok inside a compound "bad arguments"
for fn in ['irs_reg_energy', 'irs_label_boxes', 'irs_label_surface_distance', 'irs_label_hausdorff_distance']:
    case('C=max+1', fn, 'bad arguments', C=MAXC + 1)
for C_ in (0, MAXC + 1):
    case(f'C={C_}', 'irs_label_posterior_workspace', 'bad arguments', C=C_)
for fn, arg in [('irs_warp_fwd', 'Cim'), ('irs_warp_bwd', 'Cim'), ('irs_warp_transformation', 'Cim'), ('irs_warp_nearest_u8', 'Cim'),
                ('irs_warp_nearest_i16', 'Cim'), ('irs_lcc_map_fwd', 'Cf'), ('irs_lcc_map_bwd', 'Cf'), ('irs_label_boxes', 'Cf'),
                ('irs_label_surface_distance', 'Cf'), ('irs_label_hausdorff_distance', 'Cf')]:
    for n in (0, 3):  # neither 1 nor C = 2
        case(f'{arg}={n}', fn, 'bad arguments', **{arg: n})
case('mask_chains=3', 'irs_inverse_consistency', 'mask of 3 chains, 1 or 2 needed', mask=P, mask_chains=3)
case('Cim=3', 'irs_native_warp', 'moving volumes of 3 chains, 1 or 2 needed', Cim=3)
case('Cf=3', 'irs_image_similarity', 'fixed image of 3 chains, 1 or 2 needed', Cf=3)

# ---- records_ok: records_before = -1 and records_before = ceiling - C + 1 (C = 2)
for fn, ceiling, overflow in [
        ('irs_label_posterior_update', I32MAX, 'overflow the int32 record count'),
        ('irs_jacobian_posterior_update', I32MAX, 'overflow the int32 fold count'),
        ('irs_displacement_covariance_update', I32MAX, 'overflow the int32 record count'),
        ('irs_displacement_quantiles_update', L.IRS_QUANTILE_MAX_RECORDS, 'exceed the 65535 a uint16 count holds'),
        ('irs_inverse_consistency_update', I32MAX, 'overflow the int32 record count'),
        ('irs_landmark_update', I32MAX, 'overflow the int32 record count')]:
    case('records=-1', fn, 'records_before = -1 < 0', records_before=-1)
    case('records=ceiling', fn, f'{ceiling - 1} records + 2 chains {overflow}', records_before=ceiling - 2 + 1)

# ---- positive3 (and the two sites that word or order it differently): zero, negative, NaN, infinite at each position
BAD_FLOATS = [('zero', 0.0, '0'), ('neg', -1.0, '-1'), ('nan', NAN, 'nan'), ('inf', INF, 'inf')]
for fn, arg in [('irs_displacement_covariance_finalize', 'scale'), ('irs_displacement_quantiles_update', 'inv_width'),
                ('irs_displacement_quantiles_finalize', 'width'), ('irs_displacement_quantiles_finalize', 'scale'),
                ('irs_inverse_consistency', 'scale'), ('irs_transform_points', 'scale')]:
    for what, v, shown in BAD_FLOATS:
        for a in range(3):
            vals = [1.0, 1.0, 1.0]
            vals[a] = v
            case(f'{arg}[{a}]={what}', fn, f'{arg}[{a}] = {shown}, a finite value > 0 needed', **{arg: f3(*vals)})
for fn in ['irs_label_surface_distance', 'irs_label_hausdorff_distance']:
    for what, v, _ in BAD_FLOATS:
        for a in range(3):
            vals = [1.0, 1.0, 1.0]
            vals[a] = v
            case(f'spacing[{a}]={what}', fn, 'spacing must be positive', spacing=f3(*vals))
# (width is looked at before scale on every axis)
case('width[1]-before-scale[0]', 'irs_displacement_quantiles_finalize', 'scale[0] = 0, a finite value > 0 needed',
     width=f3(1, 0, 1), scale=f3(0, 1, 1))
for what, v, shown in BAD_FLOATS:
    case(f'threshold={what}', 'irs_inverse_consistency_finalize', f'threshold = {shown}, a finite value > 0 needed', threshold=v)

# ---- workspace_ok: one byte short
for fn, arg, need, hint in [
        ('irs_label_surface_distance', 'workspace_bytes', 3328, 'irs_surface_distance_workspace'),
        ('irs_label_hausdorff_distance', 'workspace_bytes', 69632, 'irs_hausdorff_workspace'),
        ('irs_split_rhat', 'ws_bytes', 40, 'irs_split_rhat_workspace'),
        ('irs_split_ess', 'ws_bytes', 40, 'irs_split_ess_workspace'),
        ('irs_label_posterior_update', 'ws_bytes', 16, 'irs_label_posterior_workspace'),
        ('irs_label_posterior_finalize', 'ws_bytes', 608, 'irs_label_posterior_workspace'),
        ('irs_jacobian_posterior_finalize', 'ws_bytes', 73728, 'IRS_JACOBIAN_WS_BYTES'),
        ('irs_displacement_covariance_finalize', 'ws_bytes', 81920, 'IRS_COVARIANCE_WS_BYTES'),
        ('irs_displacement_quantiles_finalize', 'ws_bytes', 65536, 'IRS_QUANTILE_WS_BYTES'),
        ('irs_inverse_consistency', 'ws_bytes', 327680, 'IRS_ICE_WS_BYTES'),
        ('irs_inverse_consistency_finalize', 'ws_bytes', 49152, 'IRS_ICE_MAP_WS_BYTES'),
        ('irs_landmark_finalize', 'ws_bytes', 57344, 'IRS_LANDMARK_WS_BYTES'),
        ('irs_image_similarity', 'ws_bytes', 74240, 'irs_image_similarity_workspace')]:
    assert GOOD[fn][arg] == need, fn
    case('ws-1', fn, f'workspace of {need - 1} bytes, {need} needed ({hint})', **{arg: need - 1})

# ---- label tables
for fn, n_arg in [('irs_label_boxes', 'n_labels'), ('irs_label_surface_distance', 'n_labels'),
                  ('irs_label_hausdorff_distance', 'n_labels'), ('irs_label_posterior_update', 'K'),
                  ('irs_label_posterior_finalize', 'K')]:
    msg = f'1..{L.IRS_MAX_LABELS} labels in the int16 range'
    case('labels=null', fn, msg, labels=None)
    case('labels=0', fn, msg, **{n_arg: 0})
    case('labels=max+1', fn, msg, labels=i32(*range(L.IRS_MAX_LABELS + 1)), **{n_arg: L.IRS_MAX_LABELS + 1})
    case('label=32768', fn, msg, labels=i32(1, 32768))
    case('label=-32769', fn, msg, labels=i32(-32769, 2))
for fn in ['irs_label_posterior_update', 'irs_label_posterior_finalize']:
    case('label-twice', fn, 'label 7 appears twice', labels=i32(7, 7))

# ---- average surface distance and Hausdorff distance: arguments and layout
for fn in ['irs_label_surface_distance', 'irs_label_hausdorff_distance']:
    for arg in ['seg_fixed', 'seg_moving', 'spacing', 'workspace', 'counts', 'sums'] + (['hd'] if 'hausdorff' in fn else []):
        case(f'{arg}=null', fn, 'bad arguments', **{arg: None})
    case('C=0', fn, 'bad arguments', C=0)
    case('D=1', fn, 'bad arguments', D=1)
    case('boxes=null', fn, 'irs_surface_distance: bad boxes / dims', boxes=None)
    case('box-below', fn, 'irs_surface_distance: box 0 out of the volume', boxes=i32(*([-1, 0, 0, 3, 3, 3] + [0, 0, 0, 3, 3, 3] * 3)))
    case('box-beyond', fn, 'irs_surface_distance: box 2 out of the volume', boxes=i32(*([0, 0, 0, 3, 3, 3] * 2 + [0, 0, 0, 3, 3, 4] * 2)))
    case('box-inverted', fn, 'irs_surface_distance: box 3 out of the volume', boxes=i32(*([0, 0, 0, 3, 3, 3] * 3 + [0, 2, 0, 3, 1, 3])))
case('bytes=null', 'irs_surface_distance_workspace', 'null argument', bytes=None)
case('boxes=null', 'irs_surface_distance_workspace', 'irs_surface_distance: bad boxes / dims', boxes=None)
case('pairs=0', 'irs_surface_distance_workspace', 'irs_surface_distance: bad boxes / dims', n_pairs=0)
case('W=1', 'irs_surface_distance_workspace', 'irs_surface_distance: bad boxes / dims', W=1)
case('box-beyond', 'irs_surface_distance_workspace', 'irs_surface_distance: box 0 out of the volume', boxes=i32(*([0, 0, 0, 4, 3, 3] * 4)))
case('bytes=null', 'irs_hausdorff_workspace', 'null argument', bytes=None)
case('Q=-1', 'irs_hausdorff_workspace', 'irs_label_hausdorff_distance: 0..4 percentiles, got -1', Q=-1)
case('Q=5', 'irs_hausdorff_workspace', 'irs_label_hausdorff_distance: 0..4 percentiles, got 5', Q=5)
case('boxes=null', 'irs_hausdorff_workspace', 'irs_surface_distance: bad boxes / dims', boxes=None)
case('Q=-1', 'irs_label_hausdorff_distance', '0..4 percentiles, got -1', Q=-1)
case('Q=5', 'irs_label_hausdorff_distance', '0..4 percentiles, got 5', Q=5)
case('percentiles=null', 'irs_label_hausdorff_distance', '2 percentiles need percentiles and hd_pct', percentiles=None)
case('hd_pct=null', 'irs_label_hausdorff_distance', '2 percentiles need percentiles and hd_pct', hd_pct=None)
for what, pct in [('zero', (0, 95)), ('above-100', (50, 100.5)), ('nan', (NAN, 95)), ('equal', (50, 50)), ('falling', (95, 50))]:
    case(f'percentiles-{what}', 'irs_label_hausdorff_distance', 'percentiles must lie in (0, 100] and increase strictly', percentiles=f64(*pct))

# ---- native-resolution outputs
NW = 'irs_native_warp'
for arg in ['displacement', 'dims', 'native', 'padding']:
    case(f'{arg}=null', NW, 'bad arguments', **{arg: None})
case('no-output', NW, 'no output requested', im_out=None, seg_out=None, mask_out=None, displacement_out=None)
for arg in ['im', 'seg', 'mask']:
    case(f'{arg}=null', NW, 'an output is requested of a moving volume that is NULL', **{arg: None})
case('scale=null', NW, 'displacement_out needs scale', scale=None)
case('native=0', NW, 'native[1] = 0 < 1', native=i32(6, 0, 6))
case('padding=-1', NW, 'padding[2] = -1 < 0', padding=i32(1, 1, -1))
case('extent=1', NW, 'padded extent 1 of axis 0, >= 2 needed', native=i32(1, 6, 6), padding=i32(0, 1, 1))
case('dims=1', NW, 'dims[2] = 1 < 2', dims=i32(4, 4, 1))
case('extent=2^24', NW, 'padded extent 16777216 of axis 1 is not exact in float32', native=i32(6, 1 << 24, 6), padding=i32(1, 0, 1))
case('voxels=2^30', NW, 'the native volume must have fewer than 2^30 voxels', native=i32(1024, 1024, 1024))
case('dims=2^30', NW, 'bad dims', dims=i32(1024, 1024, 1024))
case('grid-planes', NW, 'native shape (32768, 6, 6) x 2 chains exceeds the launch grid', native=i32(32768, 6, 6))
case('grid-rows', NW, 'native shape (6, 262141, 6) x 2 chains exceeds the launch grid', native=i32(6, 262141, 6))
case('scale=inf', NW, 'scale[1] = inf, a finite value needed', scale=f3(1, INF, 1))
case('scale=nan', NW, 'scale[2] = nan, a finite value needed', scale=f3(1, 1, NAN))
case('fill=nan', NW, 'fill = nan, a finite value needed', fill=NAN)
case('fill=-inf', NW, 'fill = -inf, a finite value needed', fill=-INF)

# ---- intensity similarity
IS = 'irs_image_similarity'
for arg in ['fixed', 'moving', 'stats', 'ws']:
    case(f'{arg}=null', IS, 'bad arguments', **{arg: None})
for fn in [IS, 'irs_image_similarity_workspace']:
    case('bins=1', fn, 'bins = 1, 2..128', bins=1)
    case('bins=129', fn, 'bins = 129, 2..128', bins=129)
case('bytes=null', 'irs_image_similarity_workspace', 'bad arguments', bytes=None)
case('H=0', IS, 'dims (4, 0, 4), every one >= 1 needed', H=0)
case('voxels=2^30', IS, 'the volume must have fewer than 2^30 voxels', D=1024, H=1024, W=1024)
case('fixed-empty', IS, 'fixed range [1, 1], finite bounds with hi > lo needed', f_lo=1.0, f_hi=1.0)
case('fixed-nan', IS, 'fixed range [nan, 1], finite bounds with hi > lo needed', f_lo=NAN)
case('moving-inf', IS, 'moving range [0, inf], finite bounds with hi > lo needed', m_hi=INF)
case('moving-wide', IS, 'moving range [-3e+38, 3e+38] is too wide or too narrow for float32 bins', m_lo=-3e38, m_hi=3e38)
case('fixed-narrow', IS, 'fixed range [0, 1.4013e-45] is too wide or too narrow for float32 bins', f_hi=1e-45)
case('ws-unaligned', IS, 'the workspace must be 16-byte aligned', ws=P + 8)

# ---- landmark propagation
TP = 'irs_transform_points'
for arg in ['points', 'displacement', 'scale']:
    case(f'{arg}=null', TP, 'bad arguments', **{arg: None})
case('no-output', TP, 'no output requested', sampled=None, mapped=None)
case('K=0', TP, f'K = 0 points, 1..{1 << 24}', K=0)
case('K=max+1', TP, f'K = {(1 << 24) + 1} points, 1..{1 << 24}', K=(1 << 24) + 1)
case('D=1', TP, 'bad dims (1, 4, 4)', D=1)
case('K=0', 'irs_landmark_update', f'K = 0 landmarks, 1..{1 << 24}', K=0)
case('K=0', 'irs_landmark_finalize', f'K = 0 landmarks, 1..{1 << 24}', K=0)


@pytest.fixture(scope='module')
def lib():
    return L.load()


def refused(lib, rc, expected, exact=True):
    got = lib.irs_last_error().decode()
    assert rc == 1, (rc, got)
    assert got == expected if exact else expected in got, got


@pytest.mark.parametrize('fn,bad,expected,exact', [pytest.param(*c[1:], id=c[0]) for c in CASES])
def test_refusal(lib, fn, bad, expected, exact):
    refused(lib, getattr(lib, fn)(*{**GOOD[fn], **bad}.values()), expected, exact)


def test_case_ids_are_unique():
    ids = [c[0] for c in CASES]
    assert len(ids) == len(set(ids)), sorted(i for i in ids if ids.count(i) > 1)


# ---- irs_create: the configuration is refused before anything is allocated
def _cfg(engine=None, **fields):
    c = irs_config(EngineConfig(dims=(8, 8, 8), **(engine or {})))
    for k, v in fields.items():
        if isinstance(v, tuple):
            getattr(c, k)[:] = list(v)
        else:
            setattr(c, k, v)
    return c


CREATE_CASES = [
    ('dims', _cfg(dims=(8, 1, 8)), f'irs_create: bad dims / chains (C <= {MAXC})'),
    ('voxels=2^30', _cfg(dims=(1024, 1024, 1024)), f'irs_create: bad dims / chains (C <= {MAXC})'),
    ('C=0', _cfg(no_chains=0), f'irs_create: bad dims / chains (C <= {MAXC})'),
    ('C=max+1', _cfg(no_chains=MAXC + 1), f'irs_create: bad dims / chains (C <= {MAXC})'),
    ('steps=0', _cfg(no_steps=0), 'irs_create: no_steps out of range'),
    ('steps=31', _cfg(no_steps=31), 'irs_create: no_steps out of range'),
    ('sobolev=-1', _cfg(sobolev_s=-1), 'irs_create: sobolev_s out of range'),
    ('sobolev=max+1', _cfg(sobolev_s=L.IRS_MAX_HALF_WIDTH + 1), 'irs_create: sobolev_s out of range'),
    ('data-loss', _cfg(data_loss=2), 'irs_create: unknown data loss'),
    ('lcc=0', _cfg(lcc_s=0), 'irs_create: LCC half width must be 1 or 2'),
    ('lcc=3', _cfg(lcc_s=3), 'irs_create: LCC half width must be 1 or 2'),
    ('lcc-wide', _cfg(dims=(4, 8, 8), lcc_s=2), 'irs_create: LCC half width must be 1 or 2'),
    ('components=0', _cfg(gmm_components=0), f'irs_create: 1..{L.IRS_MAX_COMPONENTS} mixture components'),
    ('components=max+1', _cfg(gmm_components=L.IRS_MAX_COMPONENTS + 1), f'irs_create: 1..{L.IRS_MAX_COMPONENTS} mixture components'),
    ('ssd-sigma=0', _cfg(dict(data_loss='SSD'), ssd_sigma=0.0), 'irs_create: ssd_sigma must be positive'),
    ('ssd-sigma=nan', _cfg(dict(data_loss='SSD'), ssd_sigma=NAN), 'irs_create: ssd_sigma must be positive'),
    ('regulariser=-1', _cfg(reg_loss=-1), 'irs_create: unknown regulariser'),
    ('regulariser=4', _cfg(reg_loss=4), 'irs_create: unknown regulariser'),
    ('student-learnable', _cfg(dict(reg_loss='RegLoss_Student'), reg_learnable=1),
     'irs_create: RegLoss_Student / RegLoss_LogNormal_L2 have no learnable parameters'),
    ('lognormal-l2-learnable', _cfg(dict(reg_loss='RegLoss_LogNormal_L2'), reg_learnable=1),
     'irs_create: RegLoss_Student / RegLoss_LogNormal_L2 have no learnable parameters'),
    ('student-prior', _cfg(dict(reg_loss='RegLoss_Student'), w_reg_prior_rate=0.0),
     'irs_create: RegLoss_Student needs a0 > 0 and b0 > 0 (w_reg_prior_shape / w_reg_prior_rate)'),
    ('cps=0', _cfg(cps=(2, 0, 2)), 'irs_create: control point spacing must be 1..8 on every axis'),
    ('cps=9', _cfg(cps=(2, 2, 9)), 'irs_create: control point spacing must be 1..8 on every axis'),
]


@pytest.mark.parametrize('cfg,expected', [pytest.param(*c[1:], id=c[0]) for c in CREATE_CASES])
def test_create_refuses_configuration(lib, cfg, expected):
    ctx = C.c_void_p()
    refused(lib, lib.irs_create(C.byref(cfg), C.byref(ctx)), expected)
    assert not ctx.value


def test_create_refuses_null(lib):
    ctx = C.c_void_p()
    refused(lib, lib.irs_create(None, C.byref(ctx)), 'irs_create: null argument')
    refused(lib, lib.irs_create(C.byref(_cfg()), None), 'irs_create: null argument')


# ---- the switches: one table behind irs_option_set and the IRS_* environment variables
def knob_fields():
    """name -> default of every field of struct Knobs (csrc/common.h)"""
    src = open(os.path.join(ROOT, 'ir_sgmcmc_amd', 'csrc', 'common.h')).read()
    body = re.search(r'struct Knobs \{(.*?)\n\};', src, re.S).group(1)
    body = re.sub(r'//[^\n]*', '', body)
    return {name: int(v) for decl in re.findall(r'\bint\s+([^;]+);', body) for name, v in re.findall(r'(\w+)\s*=\s*(-?\d+)', decl)}


KNOBS = knob_fields()
CHILD = r'''
import ctypes, sys
lib = ctypes.CDLL(sys.argv[1])  # (ctypes alone: a child per switch has no time to import more)
lib.irs_option_set.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int]
lib.irs_last_error.restype = ctypes.c_char_p
for name, value in zip(sys.argv[2::2], sys.argv[3::2]):
    assert lib.irs_option_set(None, name.encode(), int(value)) == 0, lib.irs_last_error()
print('ok')
'''


def _child(env, *args):
    env = {**{k: v for k, v in os.environ.items() if not k.startswith('IRS_')}, **env}
    out = subprocess.run([sys.executable, '-c', CHILD, L.LIB_PATH, *map(str, args)], env=env, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == 'ok', out.stderr


def test_switch_table_is_complete(lib):
    """irs_option_set accepts exactly the fields of struct Knobs: 32 of each.  (Setting a switch to the value it has changes nothing;
    the names go to a fresh process all the same, which leaves this one's switches alone.)"""
    assert len(KNOBS) == 32
    _child({}, *[x for name, default in KNOBS.items() for x in (name, default)])
    src = open(os.path.join(ROOT, 'ir_sgmcmc_amd', 'csrc', 'knobs.hip')).read()
    table = re.search(r'kSwitches\[\] = \{(.*?)\n\};', src, re.S).group(1)
    rows = re.findall(r'\{"(\w+)", &Knobs::(\w+), KN_(?:CTX|GLOBAL|LAYOUT)\}', table)
    assert sorted(n for n, _ in rows) == sorted(KNOBS) and all(n == f for n, f in rows)


def test_option_set_refusals(lib):
    refused(lib, lib.irs_option_set(None, b'no_such_switch', 1), "irs_option_set: unknown option 'no_such_switch'")
    refused(lib, lib.irs_option_set(None, b'IRS_RUN_AHEAD', 1), "irs_option_set: unknown option 'IRS_RUN_AHEAD'")
    refused(lib, lib.irs_option_set(None, None, 1), 'irs_option_set: null name')
    ctx = C.create_string_buffer(1 << 16)  # stands in for a context: a process-wide switch is refused before the context is looked at
    for name in ('sobolev_tile', 'launch_log', 'seg_fit', 'update_seg'):
        refused(lib, lib.irs_option_set(ctx, name.encode(), 1),
                f"irs_option_set: '{name}' is a process-wide switch (the launchers read it at every launch): set it with ctx == NULL")


def test_option_set_round_trip():
    """one switch of each scope, there and back, in a fresh process"""
    for name in ('run_ahead', 'fwd_pf', 'seg_min_len'):  # context, process-wide, layout
        _child({}, name, KNOBS[name] + 1, name, KNOBS[name])


@pytest.mark.parametrize('name', sorted(KNOBS))
def test_environment_names_every_switch(name):
    """IRS_<NAME> in the environment of a fresh process: the library starts, and setting the same value is accepted whatever the
    scope (no context is alive).  Nothing on the host tells whether the value was taken -- the GPU test below does."""
    value = 'b' if name == 'sobolev_tile' else str(KNOBS[name] + 1)
    _child({f'IRS_{name.upper()}': value}, name, 2 if value == 'b' else value)


GPU_CHILD = r'''
import ctypes as C, sys
import torch
from ir_sgmcmc_amd import _lib as L, ops
from ir_sgmcmc_amd.engine import EngineConfig, irs_config
lib = L.load()
layout = dict(zip(sys.argv[1::3], map(int, sys.argv[2::3])))
defaults = dict(zip(sys.argv[1::3], map(int, sys.argv[3::3])))
cfg, ctx = irs_config(EngineConfig(dims=(16, 16, 16))), C.c_void_p()
L.check(lib.irs_create(C.byref(cfg), C.byref(ctx)))
try:  # a layout switch may only be "set" to the value it has while a context is alive: that reads it back
    for name, value in layout.items():
        L.check(lib.irs_option_set(None, name.encode(), value))
        assert lib.irs_option_set(None, name.encode(), value + 1) == 1 and b'1 context(s) are alive' in lib.irs_last_error(), name
finally:
    lib.irs_destroy(ctx)
for name, value in defaults.items():  # (the launch below runs in the default layout)
    L.option_set(name, value)
im = torch.rand(1, 1, 16, 16, 16, device='cuda')
ops.lcc_normalise(im, 1)
torch.cuda.synchronize()
print('ok')
'''


@pytest.mark.gpu
def test_environment_is_read():
    """the values the environment names reach the switches: the launch log speaks, and the layout switches -- which a live context
    pins -- hold the values they were given (IRS_SOBOLEV_TILE in its letter form rides along: the library starts with it)"""
    layout = {'seg_fit': 0, 'seg_min_blocks': 512, 'seg_min_len': 4, 'lcc_seg': 8, 'stats_seg': 8, 'update_seg': 8}
    assert all(KNOBS[k] != v for k, v in layout.items())
    env = {**os.environ, 'IRS_LAUNCH_LOG': '1', 'IRS_SOBOLEV_TILE': 'b', **{f'IRS_{k.upper()}': str(v) for k, v in layout.items()},
           'PYTHONPATH': ROOT + os.pathsep + os.environ.get('PYTHONPATH', '')}
    out = subprocess.run([sys.executable, '-c', GPU_CHILD, *[str(x) for k, v in layout.items() for x in (k, v, KNOBS[k])]], env=env,
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith('ok'), out.stderr
    assert '[irs launch] {"kernel": "lcc_fwd_march_kernel"' in out.stderr, out.stderr
