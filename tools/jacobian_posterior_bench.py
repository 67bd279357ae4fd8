"""Times the Jacobian-posterior kernels (ops.jacobian_posterior_update, ops.jacobian_posterior_finalize) against a
device-to-device copy and against what the library could do for the same state before them: ops.log_det_jacobian followed by
the elementwise Welford update in torch.

Device events around every one of `--reps` calls after `--warmup` calls, per size; the figure is the median.  The input is the
identity plus a smooth random displacement per chain (a 4^3 grid of normal draws, trilinearly upsampled).  Bytes are what the
algorithm must move: the update reads 12 C B per voxel of transformation (every neighbour tap is some thread's centre tap) and
reads and writes the 12 B of state (24 B); the finalize reads the 12 B of state and the 1 B mask and writes three float32 maps
(25 B).  The copy rate is a torch copy_ of a 2 GiB buffer, counted as read + write.  Prints one JSON line per size.  Run it
under `rocprofv3 --kernel-trace --stats` for the kernel times alone.
"""
import argparse
import json
import os
import statistics
import sys

import torch

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[128, 256])
    ap.add_argument('--chains', type=int, default=2)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    dev = 'cuda:0'
    src = torch.empty(1 << 29, device=dev)  # 2 GiB
    dst = torch.empty_like(src)
    t_copy = timed(lambda: dst.copy_(src), args.reps, args.warmup)
    copy_gbs = 2 * src.numel() * 4 / t_copy / 1e9
    del src, dst
    C = args.chains
    for n in args.sizes:
        g = torch.Generator(device=dev).manual_seed(0)
        coarse = torch.randn(C, 3, 4, 4, 4, device=dev, generator=g) * 0.05
        d = torch.nn.functional.interpolate(coarse, size=(n, n, n), mode='trilinear', align_corners=True)
        lin = torch.linspace(-1.0, 1.0, n, device=dev)
        grid = torch.stack(torch.meshgrid(lin, lin, lin, indexing='ij'))  # (3, n, n, n): z, y, x
        t = (grid.flip(0)[None] + d).contiguous()  # x, y, z channels
        del d, grid
        folds = torch.zeros(n, n, n, device=dev, dtype=torch.int32)
        mean = torch.zeros(n, n, n, device=dev)
        m2 = torch.zeros(n, n, n, device=dev)
        mask = torch.ones(n, n, n, device=dev, dtype=torch.bool)
        records = [0]

        def update():
            ops.jacobian_posterior_update(t, folds, mean, m2, records[0])
            records[0] += C

        t_upd = timed(update, args.reps, args.warmup)
        n_rec = records[0]
        t_fin = timed(lambda: ops.jacobian_posterior_finalize(folds, mean, m2, n_rec, mask), args.reps, args.warmup)

        # the same state from the per-sample operator and torch elementwise kernels
        folds_b, mean_b, m2_b = torch.zeros_like(folds), torch.zeros_like(mean), torch.zeros_like(m2)
        records_b = [0]
        zero = torch.zeros((), device=dev)

        def baseline():
            _, ld = ops.log_det_jacobian(t)
            for c in range(C):
                x = ld[c]
                valid = torch.isfinite(x)
                folds_b.add_(~valid)
                k = (records_b[0] + c + 1 - folds_b).clamp_(min=1).float()
                dlt = torch.where(valid, x - mean_b, zero)
                mean_b.add_(dlt / k)
                m2_b.add_(dlt * torch.where(valid, x - mean_b, zero))
            records_b[0] += C

        t_base = timed(baseline, args.reps, args.warmup)
        V = n ** 3
        b_upd, b_fin = (12 * C + 24) * V, 25 * V
        print(json.dumps({'size': n, 'chains': C, 'copy_GBs': round(copy_gbs, 1),
                          'update_ms': round(t_upd * 1e3, 4), 'update_MB': round(b_upd / 1e6, 1),
                          'update_GBs': round(b_upd / t_upd / 1e9, 1),
                          'baseline_ms': round(t_base * 1e3, 4), 'baseline_over_update': round(t_base / t_upd, 2),
                          'finalize_ms': round(t_fin * 1e3, 4), 'finalize_MB': round(b_fin / 1e6, 1),
                          'finalize_GBs': round(b_fin / t_fin / 1e9, 1),
                          'mean_max_abs_diff_to_baseline': float((mean - mean_b).abs().max())}), flush=True)
        del t, folds, mean, m2, folds_b, mean_b, m2_b, mask


if __name__ == '__main__':
    main()
