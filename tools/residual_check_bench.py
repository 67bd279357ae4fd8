"""Times the two kernels of the residual model check -- residual_check.residual_histogram (the histogram launch and its
one-block-per-chain finish) and residual_check.residual_nll_update -- against their byte floors at the HBM rate of DESIGN.md
section 4 (8 TB/s): 5 B per voxel and chain for the histogram (z and the mask read once), 4 B per voxel and chain + 16 B per
voxel for the map (z read; mean and count read and written).  ops.image_similarity at the same shape is timed alongside: the
nearest existing kernel (9 B per voxel and chain, a 2-D histogram).

Device events around every one of `--reps` calls after `--warmup` calls; the figure is the median, and each call is timed in
two rounds that alternate with the others, the better median kept: other work shares the device.  Residuals drawn from a
four-component mixture, exactly 0 on the first half of the volume as the LCC residual of a flat background is; a mask of 60 %
of the voxels; 128 bins; K = 4.  The timed calls allocate their workspace as the trainer's calls do.  Prints one JSON line
per (size, chains).  Run it under `rocprofv3 --kernel-trace --stats` for the kernel times alone.
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ir_sgmcmc_amd import ops, residual_check  # noqa: E402

HBM_BYTES_PER_S = 8e12


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
    ap.add_argument('--chains', type=int, nargs='+', default=[1, 2])
    ap.add_argument('--bins', type=int, default=128)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    dev = 'cuda:0'
    std = [0.01, 0.04, 0.15, 0.6]
    pi = [0.4, 0.3, 0.2, 0.1]
    log_weight = [math.log(p) - math.log(s) - 0.5 * math.log(2 * math.pi) for s, p in zip(std, pi)]
    inv_std = [1.0 / s for s in std]
    g = torch.Generator(device=dev).manual_seed(0)
    for N in args.sizes:
        V = N ** 3
        mask = torch.rand(1, 1, N, N, N, device=dev, generator=g) < 0.6
        for C in args.chains:
            k = torch.multinomial(torch.tensor(pi, device=dev), C * V, replacement=True, generator=g)
            z = (torch.randn(C * V, device=dev, generator=g) * torch.tensor(std, device=dev)[k]).view(C, 1, N, N, N)
            z.view(C, -1)[:, :V // 2] = 0.0
            fixed = torch.rand(1, 1, N, N, N, device=dev, generator=g)
            moving = torch.rand(C, 1, N, N, N, device=dev, generator=g)
            state = residual_check.residual_histogram(z, mask, 1.0, args.bins)
            mean = torch.zeros(N, N, N, device=dev)
            count = torch.zeros(N, N, N, device=dev, dtype=torch.int32)
            calls = {'histogram': lambda: residual_check.residual_histogram(z, mask, 1.0, args.bins, **state, records_before=C),
                     'nll_update': lambda: residual_check.residual_nll_update(z, log_weight, inv_std, mean, count, C),
                     'image_similarity': lambda: ops.image_similarity(fixed, moving, mask, args.bins, (0.0, 1.0), (0.0, 1.0))}
            times = {name: [] for name in calls}
            for _ in range(2):
                for name, fn in calls.items():
                    times[name].append(timed(fn, args.reps, args.warmup))
            t = {name: min(v) for name, v in times.items()}
            floor = {'histogram': 5 * V * C / HBM_BYTES_PER_S, 'nll_update': (4 * C + 16) * V / HBM_BYTES_PER_S,
                     'image_similarity': (4 + 5 * C) * V / HBM_BYTES_PER_S}
            row = {'size': N, 'chains': C, 'bins': args.bins}
            for name in calls:
                row[f'{name}_us'] = round(t[name] * 1e6, 1)
                row[f'{name}_floor_us'] = round(floor[name] * 1e6, 1)
                row[f'{name}_over_floor'] = round(t[name] / floor[name], 1)
            print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
