"""Times the posterior-label-map kernels (ops.label_posterior_update, ops.label_posterior_finalize) against a device-to-device
copy.

Device events around `--reps` back-to-back calls after `--warmup` calls, per size, on the synthetic segmentation (two nested
spheres, labels 10 and 16) warped by C random smooth displacements, with the K structures of the project's structures
dict.  Bytes are what the algorithm must move: the update reads 2 B per voxel of every chain's map and reads and writes the
4-byte count of every (voxel, chain) that carries a structure (8 B); the finalize reads the K count planes, the fixed
segmentation and the mask and writes the entropy and MAP maps ((4K + 9) B per voxel).  The copy rate is a torch copy_ of a
2 GiB buffer, counted as read + write.  Prints one JSON line per size.  Run it under `rocprofv3 --kernel-trace --stats` for
the kernel times alone.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ir_sgmcmc_amd import ops  # noqa: E402
from ir_sgmcmc_amd.data_loader import synthetic_pair  # noqa: E402

STRUCTURES = [10, 11, 12, 13, 16, 17, 18, 26, 49, 50, 51, 52, 53, 54, 58]  # ConfigParser.structures_dict


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
    C, K = args.chains, len(STRUCTURES)
    for n in args.sizes:
        fixed, moving = synthetic_pair((n, n, n), seed=0)
        seg_fixed = fixed['seg'].reshape(n, n, n).to(dev)
        seg_moving = moving['seg'].reshape(1, 1, n, n, n).to(dev)
        mask = fixed['mask'].reshape(n, n, n).to(dev)
        g = torch.Generator(device=dev).manual_seed(0)
        coarse = torch.randn(C, 3, 4, 4, 4, device=dev, generator=g) * 0.05
        d = torch.nn.functional.interpolate(coarse, size=(n, n, n), mode='trilinear', align_corners=True)
        lin = torch.linspace(-1.0, 1.0, n, device=dev)
        grid = torch.stack(torch.meshgrid(lin, lin, lin, indexing='ij'))  # (3, n, n, n): z, y, x
        transformation = (grid.flip(0)[None] + d).contiguous()  # x, y, z channels, as the warp takes them
        seg = ops.warp(seg_moving, transformation)
        counts = torch.zeros(K, n, n, n, device=dev, dtype=torch.int32)
        volume = torch.zeros(K, 2, device=dev, dtype=torch.float64)
        records = [0]

        def update():
            ops.label_posterior_update(seg, STRUCTURES, counts, volume, records[0])
            records[0] += C

        t_upd = timed(update, args.reps, args.warmup)
        t_fin = timed(lambda: ops.label_posterior_finalize(counts, records[0], STRUCTURES, seg_fixed, mask), args.reps,
                      args.warmup)
        V = n ** 3
        carried = int(torch.isin(seg, torch.tensor(STRUCTURES, device=dev, dtype=torch.int16)).sum())
        b_upd, b_fin = 2 * C * V + 8 * carried, (4 * K + 9) * V
        print(json.dumps({'size': n, 'chains': C, 'structures': K, 'copy_GBs': round(copy_gbs, 1),
                          'carried_frac': round(carried / (C * V), 4),
                          'update_ms': round(t_upd * 1e3, 4), 'update_MB': round(b_upd / 1e6, 1),
                          'update_GBs': round(b_upd / t_upd / 1e9, 1),
                          'finalize_ms': round(t_fin * 1e3, 4), 'finalize_MB': round(b_fin / 1e6, 1),
                          'finalize_GBs': round(b_fin / t_fin / 1e9, 1)}), flush=True)
        del seg, counts, volume, transformation, d, grid


if __name__ == '__main__':
    main()
