"""Times one recorded step of the surface posterior (ops.surface_posterior_update) against the call whose distances it reads
(ops.label_hausdorff_distance without percentiles) on the same maps, and the finalize.

Both calls read their boxes back to size the workspace, so a call is timed with the host clock from its start to a device
synchronise after it; the figure is the median of `--reps` calls after `--warmup` calls, the two operators alternating so that
both see the same machine.  The maps are the synthetic segmentation (three nested label shells: 10, 16, 49) as the fixed map and
its warps by C random smooth displacements as the chains' maps, with the K structures of the project's structures dict.
Prints one JSON line per size.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ir_sgmcmc_amd import ops  # noqa: E402
from ir_sgmcmc_amd.data_loader import synthetic_pair  # noqa: E402

STRUCTURES = [10, 11, 12, 13, 16, 17, 18, 26, 49, 50, 51, 52, 53, 54, 58]  # ConfigParser.structures_dict


def one_call(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[128])
    ap.add_argument('--chains', type=int, default=2)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    dev = 'cuda:0'
    C = args.chains
    spacing = (1.0, 1.0, 1.0)
    for n in args.sizes:
        fixed, moving = synthetic_pair((n, n, n), seed=0)
        seg_fixed = fixed['seg'].reshape(1, 1, n, n, n).to(dev)
        seg_moving = moving['seg'].reshape(1, 1, n, n, n).to(dev)
        mask = fixed['mask'].reshape(n, n, n).to(dev)
        g = torch.Generator(device=dev).manual_seed(0)
        coarse = torch.randn(C, 3, 4, 4, 4, device=dev, generator=g) * 0.05
        d = torch.nn.functional.interpolate(coarse, size=(n, n, n), mode='trilinear', align_corners=True)
        lin = torch.linspace(-1.0, 1.0, n, device=dev)
        grid = torch.stack(torch.meshgrid(lin, lin, lin, indexing='ij'))  # (3, n, n, n): z, y, x
        seg = ops.warp(seg_moving, (grid.flip(0)[None] + d).contiguous())  # x, y, z channels, as the warp takes them
        mean = torch.zeros(n, n, n, device=dev)
        m2 = torch.zeros_like(mean)
        count = torch.zeros(n, n, n, device=dev, dtype=torch.int32)
        hausdorff = lambda: ops.label_hausdorff_distance(seg_fixed, seg, STRUCTURES, spacing, percentiles=())
        update = lambda: ops.surface_posterior_update(seg_fixed, seg, STRUCTURES, spacing, mean, m2, count)
        finalize = lambda: ops.surface_posterior_finalize(seg_fixed, STRUCTURES, mean, m2, count, (0.5, 0.9, 0.95), mask)
        for _ in range(args.warmup):
            hausdorff(), update(), finalize()
        t_hd, t_upd, t_fin = [], [], []
        for _ in range(args.reps):
            t_hd.append(one_call(hausdorff))
            t_upd.append(one_call(update))
            t_fin.append(one_call(finalize))
        med = lambda t: statistics.median(t) * 1e3
        contour = int((count > 0).sum())
        print(json.dumps({'size': n, 'chains': C, 'structures': len(STRUCTURES), 'contour_voxels': contour,
                          'hausdorff_ms': round(med(t_hd), 4), 'update_ms': round(med(t_upd), 4),
                          'update_over_hausdorff': round(med(t_upd) / med(t_hd), 3), 'finalize_ms': round(med(t_fin), 4),
                          'hausdorff_ms_min_max': [round(min(t_hd) * 1e3, 4), round(max(t_hd) * 1e3, 4)],
                          'update_ms_min_max': [round(min(t_upd) * 1e3, 4), round(max(t_upd) * 1e3, 4)]}), flush=True)


if __name__ == '__main__':
    main()
