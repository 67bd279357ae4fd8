"""Times the displacement-quantile kernels (ops.displacement_quantiles_update, ops.displacement_quantiles_finalize) against a
device-to-device copy.

Device events around every one of `--reps` calls after `--warmup` calls, per size; the figure is the median.  The input is a
smooth random displacement plus, per chain and call, white noise of `--noise` voxels, so the counts spread over the bins as a
posterior's do (the noise decides over how many bin planes the lanes of a wavefront scatter their 2-byte updates).  Bytes are
what the algorithm must move: the update reads 12 C B per voxel of displacement and the 12 B centre and reads and writes one
2-byte count per channel and chain (12 C + 12 + 12 C B when no two chains share a bin); the first update of all writes the
centre and every bin instead (12 C + 12 + 6 bins B); the finalize reads the 12 + 6 bins B of state and the 1 B mask and writes
3 P + 1 float32 planes.  The copy rate is a torch copy_ of a 2 GiB buffer, counted as read + write.  Prints one JSON line per
size.  Run it under `rocprofv3 --kernel-trace --stats` for the kernel times alone.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ir_sgmcmc_amd import ops  # noqa: E402
from ir_sgmcmc_amd.diagnostics import DisplacementQuantiles  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[128, 256])
    ap.add_argument('--chains', type=int, default=2)
    ap.add_argument('--bins', type=int, default=64)
    ap.add_argument('--bin-width', type=float, default=0.125)
    ap.add_argument('--noise', type=float, default=0.25, help='std of the per-record noise, voxels')
    ap.add_argument('--probs', type=float, nargs='+', default=[0.05, 0.5, 0.95])
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    dev = 'cuda:0'
    src = torch.empty(1 << 29, device=dev)  # 2 GiB
    dst = torch.empty_like(src)
    t_copy = timed(lambda: dst.copy_(src), args.reps, args.warmup)
    copy_gbs = 2 * src.numel() * 4 / t_copy / 1e9
    del src, dst
    C, B, P = args.chains, args.bins, len(args.probs)
    for n in args.sizes:
        g = torch.Generator(device=dev).manual_seed(0)
        coarse = torch.randn(1, 3, 4, 4, 4, device=dev, generator=g) * 0.05
        smooth = torch.nn.functional.interpolate(coarse, size=(n, n, n), mode='trilinear', align_corners=True)
        sigma = args.noise * 2.0 / (n - 1)  # voxels -> normalised coordinates
        # a few different noise draws, cycled through, so successive calls do not all hit the same bins
        xs = [(smooth + sigma * torch.randn((C, 3, n, n, n), device=dev, generator=g)).contiguous() for _ in range(4)]
        dq = DisplacementQuantiles((n, n, n), dev, bins=B, bin_width=args.bin_width)
        mask = torch.ones(n, n, n, device=dev, dtype=torch.bool)
        calls = [0]

        def first():
            ops.displacement_quantiles_update(xs[0], dq.centre, dq.hist, dq.inv_width, 0)

        def update():
            calls[0] += 1
            ops.displacement_quantiles_update(xs[calls[0] % len(xs)], dq.centre, dq.hist, dq.inv_width, calls[0] * C)

        t_first = timed(first, max(args.reps // 5, 3), 2)
        t_upd = timed(update, args.reps, args.warmup)
        n_rec = (calls[0] + 1) * C
        t_fin = timed(lambda: ops.displacement_quantiles_finalize(dq.centre, dq.hist, n_rec, dq.width, dq.scale, args.probs, mask),
                      max(args.reps // 5, 3), 2)
        _, _, isum, _ = ops.displacement_quantiles_finalize(dq.centre, dq.hist, n_rec, dq.width, dq.scale, args.probs, mask)
        V = n ** 3
        b_first, b_upd, b_fin = (12 * C + 12 + 6 * B) * V, (24 * C + 12) * V, (12 + 6 * B + 1 + 4 * (3 * P + 1)) * V
        voxels, out_of_range, clipped = isum.tolist()
        print(json.dumps({'size': n, 'chains': C, 'bins': B, 'probs': P, 'noise_voxels': args.noise, 'records': n_rec,
                          'state_MB': round(dq.state_bytes() / 1e6, 1), 'copy_GBs': round(copy_gbs, 1),
                          'first_update_ms': round(t_first * 1e3, 4), 'first_update_MB': round(b_first / 1e6, 1),
                          'first_update_GBs': round(b_first / t_first / 1e9, 1),
                          'update_ms': round(t_upd * 1e3, 4), 'update_MB': round(b_upd / 1e6, 1),
                          'update_GBs': round(b_upd / t_upd / 1e9, 1),
                          'update_over_copy_rate': round(b_upd / t_upd / 1e9 / copy_gbs, 3),
                          'finalize_ms': round(t_fin * 1e3, 4), 'finalize_MB': round(b_fin / 1e6, 1),
                          'finalize_GBs': round(b_fin / t_fin / 1e9, 1),
                          'finalize_over_copy_rate': round(b_fin / t_fin / 1e9 / copy_gbs, 3),
                          'out_of_range_frac': out_of_range / voxels, 'clipped_frac': clipped / (3 * n_rec * voxels)}), flush=True)
        del xs, dq, mask


if __name__ == '__main__':
    main()
