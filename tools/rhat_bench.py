"""Times the split-R-hat kernels (ops.chain_moments_update, ops.split_rhat) against a device-to-device copy.

Device events around `--reps` back-to-back calls after `--warmup` calls, per size.  Bytes are what the algorithm must
move: the update reads the sample and the half's mean / m2 and writes mean / m2 (20 B per element of C*3*D*H*W); the
finalize reads both halves' mean / m2 and the mask and writes the map (48*C + 5 B per voxel).  The copy rate is a
torch copy_ of a 2 GiB buffer, counted as read + write.  Prints one JSON line per size.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ir_sgmcmc_amd import ops  # noqa: E402


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e-3  # seconds per call


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
        x = torch.randn(C, 3, n, n, n, device=dev, generator=g)
        mean = torch.zeros(2, C, 3, n, n, n, device=dev)
        m2 = torch.zeros_like(mean)
        for k in (1, 2):  # a state with some spread
            ops.chain_moments_update(x * k, mean, m2, 0, k)
            ops.chain_moments_update(x + k, mean, m2, 1, k)
        mask = torch.rand(n, n, n, device=dev, generator=g) < 0.5
        t_upd = timed(lambda: ops.chain_moments_update(x, mean, m2, 1, 3), args.reps, args.warmup)
        t_fin = timed(lambda: ops.split_rhat(mean, m2, 3, mask), args.reps, args.warmup)
        V = n ** 3
        b_upd, b_fin = 20 * C * 3 * V, (48 * C + 5) * V
        print(json.dumps({'size': n, 'chains': C, 'copy_GBs': round(copy_gbs, 1),
                          'update_ms': round(t_upd * 1e3, 4), 'update_GBs': round(b_upd / t_upd / 1e9, 1),
                          'finalize_ms': round(t_fin * 1e3, 4), 'finalize_GBs': round(b_fin / t_fin / 1e9, 1)}), flush=True)
        del x, mean, m2, mask


if __name__ == '__main__':
    main()
