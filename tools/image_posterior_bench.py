"""Times the image-posterior update (image_posterior.image_posterior_update: S volumes carried through C transformations in one
fused launch) against the unfused composition of existing operators: ops.warp per volume plus the elementwise Welford / min / max
update in torch on the warped copies.

Device events around every one of `--reps` calls after `--warmup` calls, per size and volume count; the figure is the median.
The input is the identity plus a smooth random displacement per chain (a 4^3 grid of normal draws, trilinearly upsampled), the
volumes uniform noise.  Bytes the fused update moves per voxel: the state is read and written once, 32 S B; the
transformation is read once per group of two volumes (a thread carries two), 12 C ceil(S / 2) B; the gather reads S C x 8 taps,
of which neighbouring threads share all but about one new 4-byte voxel per (volume, chain) under a smooth map: 4 S C B of
compulsory traffic.  `first_update_ms` times the same launch at records_before = 0, where the state is only written (16 S B):
the difference to the steady update is the cost of the state reads.  Prints one JSON line per case.  Run it under
`rocprofv3 --kernel-trace --stats` for the kernel times alone.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ir_sgmcmc_amd import image_posterior as IP  # noqa: E402
from ir_sgmcmc_amd import ops  # noqa: E402

GROUP = 2  # volumes per thread of the update kernel (csrc/kernels.h: kImagePosteriorGroup)


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
    ap.add_argument('--volumes', type=int, nargs='+', default=[1, 4, 8])
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
        for S in args.volumes:
            volumes = torch.rand(S, 1, n, n, n, device=dev, generator=g)
            state = IP.image_posterior_state(S, (n, n, n), dev)
            records = [0]

            def update():
                IP.image_posterior_update(volumes, t, state, records[0])
                records[0] += C

            update()  # the steady update reads the state: records_before > 0 from here on
            t_upd = timed(update, args.reps, args.warmup)
            t_first = timed(lambda: IP.image_posterior_update(volumes, t, state, 0), args.reps, args.warmup)

            # the same state from ops.warp per volume and torch elementwise kernels on the warped copies
            base = {k: torch.zeros_like(v) for k, v in state.items()}
            records_b = [0]

            def baseline():
                for s in range(S):
                    warped = ops.warp(volumes[s:s + 1], t)
                    for c in range(C):
                        x = warped[c, 0]
                        k = records_b[0] + c + 1
                        if k == 1:
                            base['mean'][s].copy_(x)
                            base['m2'][s].zero_()
                            base['low'][s].copy_(x)
                            base['high'][s].copy_(x)
                            continue
                        dlt = x - base['mean'][s]
                        base['mean'][s].add_(dlt / k)
                        base['m2'][s].add_(dlt * (x - base['mean'][s]))
                        torch.minimum(base['low'][s], x, out=base['low'][s])
                        torch.maximum(base['high'][s], x, out=base['high'][s])
                records_b[0] += C

            t_base = timed(baseline, args.reps, args.warmup)
            # both took warmup + reps steps of the same records (the fused one one more): compare the extremes, which do not
            # depend on the number of records
            agree = bool(torch.equal(state['low'], base['low']) and torch.equal(state['high'], base['high']))
            V = n ** 3
            b_state, b_field, b_gather = 32 * S * V, 12 * C * ((S + GROUP - 1) // GROUP) * V, 4 * S * C * V
            total = b_state + b_field + b_gather
            print(json.dumps({'size': n, 'volumes': S, 'chains': C, 'copy_GBs': round(copy_gbs, 1),
                              'update_ms': round(t_upd * 1e3, 4), 'first_update_ms': round(t_first * 1e3, 4),
                              'unfused_ms': round(t_base * 1e3, 4), 'unfused_over_update': round(t_base / t_upd, 2),
                              'state_MB': round(b_state / 1e6, 1), 'transformation_MB': round(b_field / 1e6, 1),
                              'gather_MB': round(b_gather / 1e6, 1), 'state_share_of_bytes': round(b_state / total, 3),
                              'update_GBs': round(total / t_upd / 1e9, 1),
                              'time_at_copy_rate_ms': round(total / (copy_gbs * 1e9) * 1e3, 4),
                              'extremes_equal_unfused': agree}), flush=True)
            del volumes, state, base
        del t


if __name__ == '__main__':
    main()
