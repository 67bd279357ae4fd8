"""Times the displacement-covariance kernels (ops.displacement_covariance_update, ops.displacement_covariance_finalize) against
a device-to-device copy and against what the library could do for the same state before them: the elementwise Welford update
of the mean and the six co-moments in torch, chain by chain.

Device events around every one of `--reps` calls after `--warmup` calls, per size; the figure is the median.  The input is a
smooth random displacement plus white noise per chain.  Bytes are what the algorithm must move: the update reads 12 C B per
voxel of displacement and reads and writes the 36 B of state (72 + 12 C B); the finalize reads the 36 B of state and the 1 B
mask and writes seven float32 planes (65 B).  The copy rate is a torch copy_ of a 2 GiB buffer, counted as read + write.  Prints
one JSON line per size.  Run it under `rocprofv3 --kernel-trace --stats` for the kernel times alone (`--reps 25` then gives
25 timed calls per kernel and size after the warm-up).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ir_sgmcmc_amd import ops  # noqa: E402

PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))


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
    ap.add_argument('--no-baseline', action='store_true', help='leave the torch composition out (kernel traces)')
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
        x = torch.nn.functional.interpolate(coarse, size=(n, n, n), mode='trilinear', align_corners=True)
        x = (x + 0.01 * torch.randn(x.shape, device=dev, generator=g)).contiguous()
        mean = torch.zeros(3, n, n, n, device=dev)
        com = torch.zeros(6, n, n, n, device=dev)
        mask = torch.ones(n, n, n, device=dev, dtype=torch.bool)
        scale = ((n - 1) / 2,) * 3
        records = [0]

        def update():
            ops.displacement_covariance_update(x, mean, com, records[0])
            records[0] += C

        t_upd = timed(update, args.reps, args.warmup)
        n_rec = records[0]
        t_fin = timed(lambda: ops.displacement_covariance_finalize(mean, com, n_rec, scale, mask), args.reps, args.warmup)
        V = n ** 3
        b_upd, b_fin = (72 + 12 * C) * V, 65 * V
        out = {'size': n, 'chains': C, 'copy_GBs': round(copy_gbs, 1),
               'update_ms': round(t_upd * 1e3, 4), 'update_MB': round(b_upd / 1e6, 1), 'update_GBs': round(b_upd / t_upd / 1e9, 1),
               'update_over_copy_rate': round(b_upd / t_upd / 1e9 / copy_gbs, 3),
               'finalize_ms': round(t_fin * 1e3, 4), 'finalize_MB': round(b_fin / 1e6, 1),
               'finalize_GBs': round(b_fin / t_fin / 1e9, 1)}
        if not args.no_baseline:
            # the same state from torch elementwise kernels, the trainer's own Welford convention extended to the co-moments
            mean_b, com_b = torch.zeros_like(mean), torch.zeros_like(com)
            records_b = [0]

            def baseline():
                for c in range(C):
                    records_b[0] += 1
                    delta = x[c] - mean_b
                    mean_b.add_(delta / records_b[0])
                    e = x[c] - mean_b
                    for j, (a, b) in enumerate(PAIRS):
                        com_b[j].addcmul_(delta[a], e[b])

            t_base = timed(baseline, args.reps, args.warmup)
            out.update({'baseline_ms': round(t_base * 1e3, 4), 'baseline_over_update': round(t_base / t_upd, 2)})
            del mean_b, com_b
        print(json.dumps(out), flush=True)
        del x, mean, com, mask


if __name__ == '__main__':
    main()
