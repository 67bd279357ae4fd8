"""Times native_posterior.native_posterior_update (the fused upsample, warp and fold onto the image's own voxel grid) against the
composition of the operators that exist without it, for the same state: ops.native_warp(seg, im), ops.label_posterior_update on
the native extents, and the Welford mean / M2 / min / max of the warped image as torch ops on the device.

One process.  After `--warmup` calls of each, the two alternate `--repeats` times; every window is `--calls` back-to-back calls
between two device events (the default makes a window of the faster one several tenths of a second), and the figure of a window
is its time per call.  Reported: the median, the smallest and the largest window of each, the ratio of the medians, and whether
the fused launch is faster by more than the spread (its slowest window against the composition's fastest).  Native 182 x 218 x
182, `dims` 128^3, C = 2 chains sharing the moving volumes, K = 15 structures.  The field is smooth random (about +-3 native
voxels), the image uniform random, the segmentation 4^3 blocks of the labels 0 .. 15.  Every call folds with records_before = 2,
so neither side takes the overwrite path.

Bytes are what the algorithm must move per recorded step, computed from the shapes (V native voxels, Vm grid voxels): the field
read once (12 C Vm), the moving image and segmentation read once (6 V), one count plane read and written per chain and voxel
(8 C V), the four planes of the image state read and written (32 V).  The composition moves the warped volumes on top of that:
6 C V written and 6 C V read again.  Prints one JSON line; tools/ scripts write nothing but stdout.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ir_sgmcmc_amd import native_posterior as P  # noqa: E402
from ir_sgmcmc_amd import ops  # noqa: E402
from ir_sgmcmc_amd.native import NativeGrid  # noqa: E402


def window(fn, calls):
    """seconds per call over `calls` back-to-back calls between two device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--native', type=int, nargs=3, default=[182, 218, 182])
    ap.add_argument('--dims', type=int, nargs=3, default=[128, 128, 128])
    ap.add_argument('--chains', type=int, default=2)
    ap.add_argument('--labels', type=int, default=15)
    ap.add_argument('--calls', type=int, default=1000)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=20)
    args = ap.parse_args()
    dev = 'cuda:0'
    C, K = args.chains, args.labels
    grid = NativeGrid.from_shape(args.native, args.dims)
    n, m = grid.shape, grid.dims
    g = torch.Generator(device=dev).manual_seed(0)
    u = F.interpolate(torch.randn(C, 3, 4, 4, 4, device=dev, generator=g) * 0.012, size=m, mode='trilinear',
                      align_corners=True).contiguous()
    im = torch.rand(1, 1, *n, device=dev, generator=g)
    blocks = torch.randint(0, K + 1, (1, 1, *[(k + 3) // 4 for k in n]), device=dev, generator=g)
    seg = blocks.repeat_interleave(4, 2).repeat_interleave(4, 3).repeat_interleave(4, 4)[..., :n[0], :n[1], :n[2]]
    seg = seg.to(torch.int16).contiguous()
    labels = list(range(1, K + 1))
    fill = float(im.min())
    before = 2

    fused_state = P.native_posterior_state(grid, labels, True, dev)
    comp = P.native_posterior_state(grid, labels, True, dev)

    def fused():
        P.native_posterior_update(u, grid, fused_state, before, seg=seg, im=im, fill=fill)

    def composition():
        out = ops.native_warp(u, grid, im=im, seg=seg, fill=fill)
        ops.label_posterior_update(out['seg'], labels, comp['counts'], comp['volume'], before)
        for c in range(C):
            x = out['im'][c, 0]
            d = x - comp['mean']
            comp['mean'] += d / float(before + c + 1)
            comp['m2'] += d * (x - comp['mean'])
            torch.minimum(comp['low'], x, out=comp['low'])
            torch.maximum(comp['high'], x, out=comp['high'])

    # the two fold the same records: one call each on zeroed states must agree in the counts
    fused()
    composition()
    counts_equal = bool(torch.equal(fused_state['counts'], comp['counts']))
    for _ in range(args.warmup):
        fused()
        composition()
    t_fused, t_comp = [], []
    for _ in range(args.repeats):
        t_fused.append(window(fused, args.calls))
        t_comp.append(window(composition, args.calls))
    V, Vm = n[0] * n[1] * n[2], m[0] * m[1] * m[2]
    moved_fused = 12 * C * Vm + V * (6 + 8 * C + 32)
    moved_comp = moved_fused + 12 * C * V
    med_f, med_c = statistics.median(t_fused), statistics.median(t_comp)
    ms = lambda t: round(t * 1e3, 4)
    print(json.dumps({'native': list(n), 'dims': list(m), 'chains': C, 'labels': K, 'calls_per_window': args.calls,
                      'windows': args.repeats, 'counts_equal': counts_equal,
                      'fused_ms': ms(med_f), 'fused_min_ms': ms(min(t_fused)), 'fused_max_ms': ms(max(t_fused)),
                      'composition_ms': ms(med_c), 'composition_min_ms': ms(min(t_comp)), 'composition_max_ms': ms(max(t_comp)),
                      'composition_over_fused': round(med_c / med_f, 3),
                      'faster_by_more_than_the_spread': bool(max(t_fused) < min(t_comp)),
                      'window_seconds': [round(med_f * args.calls, 3), round(med_c * args.calls, 3)],
                      'fused_moved_MB': round(moved_fused / 1e6, 1), 'composition_moved_MB': round(moved_comp / 1e6, 1),
                      'fused_GBs': round(moved_fused / med_f / 1e9, 1), 'composition_GBs': round(moved_comp / med_c / 1e9, 1),
                      'intermediates_avoided_MB': round(6 * C * V / 1e6, 1)}), flush=True)


if __name__ == '__main__':
    main()
