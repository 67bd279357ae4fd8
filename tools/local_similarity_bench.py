"""Times ops.local_similarity (windowed LNCC and SSIM maps in one fused launch) against the torch composition a user would write
for the same maps -- five avg_pool3d over replicate-padded float64 tensors, then the two formulas -- and against the
streaming floor: 8 B read and 8 B written per voxel and chain at the rate of a device-to-device copy measured here.

Device events around every one of `--reps` calls after `--warmup` calls; the figure is the median.  One chain, uniform-noise
images with moving = 0.6 fixed + 0.4 noise, ranges given so that the call does not synchronise, both maps written.  The call
is the map kernel plus its one-block second stage.  The copy rate is a torch copy_ of a 2 GiB buffer, counted as read +
write.  Prints one JSON line per (size, radius).  Run it under `rocprofv3 --kernel-trace --stats` for the kernel time alone.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ir_sgmcmc_amd import ops  # noqa: E402


def timed(fn, reps, warmup):
    """median seconds per call"""
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    torch.cuda.synchronize()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev) * 1e-3


def composition(fixed, moving, r, consts):
    """the maps of ops.local_similarity from torch operators, in float64"""
    floor_f, floor_m, c1, c2 = consts
    pad = lambda t: F.pad(t, (r,) * 6, mode='replicate')
    mean = lambda t: F.avg_pool3d(pad(t), 2 * r + 1, stride=1)
    f, m = fixed.double(), moving.double()
    mu_f, mu_m, e_ff, e_mm, e_fm = mean(f), mean(m), mean(f * f), mean(m * m), mean(f * m)
    var_f, var_m = (e_ff - mu_f * mu_f).clamp_min(0.0), (e_mm - mu_m * mu_m).clamp_min(0.0)
    cov = e_fm - mu_f * mu_m
    lncc = (cov / (var_f * var_m).sqrt()).clamp(-1.0, 1.0)
    lncc = lncc.where((var_f > floor_f) & (var_m > floor_m), lncc.new_full((), float('nan')))
    ssim = ((2.0 * mu_f * mu_m + c1) * (2.0 * cov + c2)) / ((mu_f * mu_f + mu_m * mu_m + c1) * (var_f + var_m + c2))
    return {'lncc': lncc.float(), 'ssim': ssim.float()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[128, 256])
    ap.add_argument('--radii', type=int, nargs='+', default=[2, 4])
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    dev = 'cuda:0'
    src = torch.empty(1 << 29, device=dev)  # 2 GiB
    dst = torch.empty_like(src)
    t_copy = timed(lambda: dst.copy_(src), args.reps, args.warmup)
    copy_gbs = 2 * src.numel() * 4 / t_copy / 1e9
    del src, dst
    unit = (0.0, 1.0)
    consts = ops.local_similarity_constants(unit, unit)
    g = torch.Generator(device=dev).manual_seed(0)
    for N in args.sizes:
        fixed = torch.rand(1, 1, N, N, N, device=dev, generator=g)
        moving = (0.6 * fixed + 0.4 * torch.rand(1, 1, N, N, N, device=dev, generator=g)).contiguous()
        for r in args.radii:
            hip = lambda: ops.local_similarity(fixed, moving, None, r, unit, unit)
            ref = lambda: composition(fixed, moving, r, consts)
            a, b = hip(), ref()
            diff = {k: float((a[k] - b[k]).abs().max()) for k in ('lncc', 'ssim')}
            del a, b
            # alternate the two, twice, and keep the better median of each: other work shares the device
            t_hip, t_torch = [], []
            for _ in range(2):
                t_hip.append(timed(hip, args.reps, args.warmup))
                t_torch.append(timed(ref, max(args.reps // 5, 3), 2))
            t_hip, t_torch = min(t_hip), min(t_torch)
            moved = 16 * N ** 3
            print(json.dumps({'size': N, 'radius': r, 'copy_GBs': round(copy_gbs, 1), 'local_similarity_ms': round(t_hip * 1e3, 4),
                              'streaming_floor_ms': round(moved / copy_gbs / 1e6, 4),
                              'fraction_of_streaming_floor': round(moved / copy_gbs / 1e9 / t_hip, 4),
                              'voxels_per_us': round(N ** 3 / t_hip / 1e6, 1), 'torch_composition_ms': round(t_torch * 1e3, 3),
                              'torch_over_local_similarity': round(t_torch / t_hip, 1), 'lncc_max_abs_diff': diff['lncc'],
                              'ssim_max_abs_diff': diff['ssim']}), flush=True)


if __name__ == '__main__':
    main()
