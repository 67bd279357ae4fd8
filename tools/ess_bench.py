"""Times the split-ESS kernels (ops.chain_variogram_update, ops.split_ess) against a device-to-device copy.

Device events around `--reps` back-to-back calls after `--warmup` calls, per (size, max_lag).  The update runs with a full
window (k - 1 >= L, so every lag is read); the finalize runs on lag sums whose rho_t = 0.9^t never gives a negative pair,
so every voxel scans all L lags (the upper bound; a real posterior stops earlier).  Bytes are what the algorithm must move,
with E = 3*D*H*W and Lt = min(k - 1, L) = L:
  update   E * (4C + 4C*Lt + 8*Lt + 4C): the sample, Lt ring slots, Lt lag sums read and written, the sample into the ring;
  finalize (48C + 12L + 9) B per voxel: both halves' mean / m2, L lag sums per component, the mask, the two maps.
The copy rate is a torch copy_ of a 2 GiB buffer, counted as read + write.  Prints one JSON line per (size, max_lag).
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
    ap.add_argument('--lags', type=int, nargs='+', default=[16, 32])
    ap.add_argument('--chains', type=int, default=2)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--transition', action='store_true',
                    help="also time one engine call (every chain one transition) at the largest size, bench.py's workload")
    args = ap.parse_args()
    dev = 'cuda:0'
    src = torch.empty(1 << 29, device=dev)  # 2 GiB
    dst = torch.empty_like(src)
    t_copy = timed(lambda: dst.copy_(src), args.reps, args.warmup)
    copy_gbs = 2 * src.numel() * 4 / t_copy / 1e9
    del src, dst
    C = args.chains
    for n in args.sizes:
        V = n ** 3
        E = 3 * V
        g = torch.Generator(device=dev).manual_seed(0)
        x = torch.randn(C, 3, n, n, n, device=dev, generator=g)
        mask = torch.rand(n, n, n, device=dev, generator=g) < 0.5
        for L in args.lags:
            ring = torch.randn(L, C, 3, n, n, n, device=dev, generator=g)
            vsum = torch.zeros(L, 3, n, n, n, device=dev)
            k = L + 1  # a full window: lags 1 .. L
            t_upd = timed(lambda: ops.chain_variogram_update(x, ring, vsum, k), args.reps, args.warmup)
            # finalize input: W = 1, B = 0 (var+ = (h - 1) / h), lag sums with rho_t = 0.9^t, h = L + 1 samples per half
            h = L + 1
            mean = torch.zeros(2, C, 3, n, n, n, device=dev)
            m2 = torch.full_like(mean, float(h - 1))
            var_plus = (h - 1) / h
            for t in range(1, L + 1):
                vsum[t - 1].fill_(2.0 * var_plus * 2 * C * (h - t) * (1.0 - 0.9 ** t))
            t_fin = timed(lambda: ops.split_ess(mean, m2, vsum, h, mask), args.reps, args.warmup)
            b_upd = E * (4 * C + 4 * C * L + 8 * L + 4 * C)
            b_fin = (48 * C + 12 * L + 9) * V
            print(json.dumps({'size': n, 'chains': C, 'max_lag': L, 'copy_GBs': round(copy_gbs, 1),
                              'update_ms': round(t_upd * 1e3, 4), 'update_GB': round(b_upd / 1e9, 2),
                              'update_GBs': round(b_upd / t_upd / 1e9, 1),
                              'finalize_ms': round(t_fin * 1e3, 4), 'finalize_GBs': round(b_fin / t_fin / 1e9, 1)}),
                  flush=True)
            del ring, vsum, mean, m2
            torch.cuda.empty_cache()
        del x, mask
    if args.transition:
        import bench
        n = max(args.sizes)
        r = bench.side_run(n, 'gmm', 'identity', 3.0, 20, 3, dev, chains=C)
        print(json.dumps({'size': n, 'chains': C, 'transition_call_ms': round(r['ms_per_transition'] * C, 4),
                          'repetitions_ms_per_chain': r['repetitions_ms']}), flush=True)


if __name__ == '__main__':
    main()
