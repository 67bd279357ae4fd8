"""Times the cubic B-spline output resampling (ir_sgmcmc_amd/bspline.py) next to the trilinear operators it stands beside.

Device events around every one of `--reps` calls after `--warmup` calls; the figure is the median.  One volume, one chain.
  - bspline.prefilter at 256^3 and at 182 x 218 x 182 (the three axis passes together);
  - bspline.warp next to ops.warp at 256^3, under a smooth random transformation (about +-3 voxels);
  - bspline.native_warp_cubic next to the image-only ops.native_warp at 182 x 218 x 182 from a 128^3 grid.
Bytes of a prefilter pass: the two sweeps of a line read the samples, write c+, read c+ back and write c -- 16 B per voxel
requested, of which 8 B per voxel (every sample read once, every coefficient written once) is what any prefilter must move.
Prints one JSON line.

The axis passes are separate launches inside one call, so events cannot part them: run the script under
`rocprofv3 --kernel-trace --output-format csv` with `--only prefilter` and give the kernel trace to `--trace FILE`, which
prints the median device time of each pass (the y and z passes share a kernel and are told apart by their grids).
"""
import argparse
import csv
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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


def smooth(C, ch, dims, amp, dev, seed):
    g = torch.Generator().manual_seed(seed)
    return (amp * F.interpolate(torch.randn(C, ch, 4, 4, 4, generator=g), size=dims, mode='trilinear', align_corners=True)).to(dev)


def passes(trace, warmup):
    """kernel trace of a `--only prefilter` run -> median microseconds per (volume, pass), the first `warmup` calls dropped"""
    rows = {}
    with open(trace, newline='') as f:
        for r in csv.DictReader(f):
            name = r['Kernel_Name']
            if 'bspline_' not in name:
                continue
            gx, gy = int(r['Grid_Size_X']), int(r['Grid_Size_Y'])
            axis = 'x' if 'bspline_x_kernel' in name else ('y' if gy > 1 else 'z')
            rows.setdefault(axis, []).append((int(r['Start_Timestamp']), (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) * 1e-3,
                                              gx * gy))
    out = {}
    for axis, calls in rows.items():
        calls.sort()
        for size in sorted({c[2] for c in calls}):  # one launch size per volume
            t = [c[1] for c in calls if c[2] == size][warmup:]
            out[f'{axis}_pass_us[{size} threads]'] = round(statistics.median(t), 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--only', choices=['prefilter'], default=None)
    ap.add_argument('--trace', default=None, help='a rocprofv3 kernel trace (csv) of a --only prefilter run: print the per-pass medians')
    args = ap.parse_args()
    if args.trace:
        print(json.dumps(passes(args.trace, args.warmup)))
        return
    from ir_sgmcmc_amd import bspline, ops
    from ir_sgmcmc_amd.native import NativeGrid
    dev = 'cuda:0'
    res = {'reps': args.reps, 'warmup': args.warmup}
    volumes = {'256^3': (256, 256, 256), '182x218x182': (182, 218, 182)}
    ims = {k: torch.rand(1, 1, *v, device=dev) for k, v in volumes.items()}
    for key, im in ims.items():
        out = torch.empty_like(im)
        call = lambda: ops._call('irs_bspline_prefilter', im.data_ptr(), out.data_ptr(), 1, *im.shape[2:])
        t = timed(call, args.reps, args.warmup)
        V = im.numel()
        res[f'prefilter {key}'] = {'ms': round(t * 1e3, 4), 'GB/s of 48 B/voxel requested': round(48 * V / t * 1e-9, 1),
                                   'GB/s of 24 B/voxel needed': round(24 * V / t * 1e-9, 1)}
    if args.only is None:
        im = ims['256^3']
        dims = volumes['256^3']
        lin = [torch.linspace(-1, 1, n, device=dev) for n in dims]
        z, y, x = torch.meshgrid(*lin, indexing='ij')
        t = (torch.stack((x, y, z)).unsqueeze(0) + smooth(1, 3, dims, 6.0 / 255, dev, 1)).contiguous()
        coeff = bspline.prefilter(im)
        res['warp 256^3'] = {'trilinear_ms': round(timed(lambda: ops.warp(im, t), args.reps, args.warmup) * 1e3, 4),
                             'cubic_ms': round(timed(lambda: bspline.warp(coeff, t), args.reps, args.warmup) * 1e3, 4)}
        native, gdims = volumes['182x218x182'], (128, 128, 128)
        grid = NativeGrid.from_shape(native, gdims)
        u = smooth(1, 3, gdims, 6.0 / 217, dev, 2).contiguous()
        nim = ims['182x218x182']
        ncoeff = bspline.prefilter(nim)
        fill = float(nim.min())
        res['native 182x218x182 from 128^3'] = {
            'trilinear_ms': round(timed(lambda: ops.native_warp(u, grid, im=nim, fill=fill), args.reps, args.warmup) * 1e3, 4),
            'cubic_ms': round(timed(lambda: bspline.native_warp_cubic(u, grid, nim, ncoeff, fill), args.reps, args.warmup) * 1e3, 4)}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
