"""Times the known-transformation validation kernels (truth.truth_update, truth.truth_calibrate) beside
ops.displacement_covariance_update on the same samples, in the same run.

Device events around every one of `--reps` calls after `--warmup` calls, per size, in `--rounds` rounds with the order of the
kernels alternating; the figure is the median over all calls and `spread` the largest relative distance of a round's median
from it.  The input is a smooth random displacement plus white noise per chain, the truth another smooth field.  Bytes are what
the algorithm must move per voxel: the truth update reads 12 C B of displacement, 12 B of truth and a 1 B mask and reads and
writes the 6 B of rank counts (25 + 12 C); the covariance update reads 12 C B and reads and writes 36 B of state (72 + 12 C);
the calibration reads 36 + 6 + 12 + 1 B and writes two float32 maps (63 B).  Prints one JSON line per size.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ir_sgmcmc_amd import ops, truth as T  # noqa: E402


def times(fn, reps, warmup):
    """seconds of each of `reps` calls"""
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    torch.cuda.synchronize()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1e-3 for a, b in ev]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[128])
    ap.add_argument('--chains', type=int, default=2)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=4)
    args = ap.parse_args()
    dev, C = 'cuda:0', args.chains
    for n in args.sizes:
        g = torch.Generator(device=dev).manual_seed(0)
        smooth = lambda k, amp: torch.nn.functional.interpolate(torch.randn(k, 3, 4, 4, 4, device=dev, generator=g) * amp,
                                                                size=(n, n, n), mode='trilinear', align_corners=True)
        truth = smooth(1, 2.0)[0].contiguous()
        x = (truth + smooth(C, 0.2) + 0.1 * torch.randn((C, 3, n, n, n), device=dev, generator=g)).contiguous()
        mask = torch.ones(n, n, n, device=dev, dtype=torch.bool)
        below = T.new_below((n, n, n), dev)
        ws = T.TruthWorkspace(dev)
        out = (torch.empty((C, 2), device=dev, dtype=torch.int64), torch.empty((C, 3), device=dev, dtype=torch.float64))
        mean, com = torch.zeros(3, n, n, n, device=dev), torch.zeros(6, n, n, n, device=dev)
        state = {'records': 0}

        def truth_update():  # (records_before stays at 1: the counts are read and written, and never overflow)
            T.truth_update(x, truth, below, 1, mask=mask, out=out, workspace=ws)

        def covariance_update():
            ops.displacement_covariance_update(x, mean, com, state['records'])
            state['records'] += C

        n_rec = 64
        edges, levels = T.calibration_thresholds(n_rec, (0.5, 0.9, 0.95), 20)
        var_edges = T.default_var_edges(16)

        def calibrate():
            T.truth_calibrate(mean, com, below, truth, n_rec, (1.0, 1.0, 1.0), edges, levels, 16, var_edges, 1e-3, mask, workspace=ws)

        fns = {'truth_update': truth_update, 'covariance_update': covariance_update, 'truth_calibrate': calibrate}
        samples = {k: [] for k in fns}
        for r in range(args.rounds):
            order = list(fns) if r % 2 == 0 else list(fns)[::-1]
            if r == 0:  # a state to calibrate
                for _ in range(n_rec // C):
                    covariance_update()
                T.truth_update(x, truth, below, 0, mask=mask, out=out, workspace=ws)
            for k in order:
                samples[k].append(times(fns[k], args.reps, args.warmup))
        V = n ** 3
        nbytes = {'truth_update': (25 + 12 * C) * V, 'covariance_update': (72 + 12 * C) * V, 'truth_calibrate': 63 * V}
        res = {'size': n, 'chains': C, 'reps': args.reps, 'rounds': args.rounds}
        for k, rounds in samples.items():
            med = statistics.median(t for r in rounds for t in r)
            spread = max(abs(statistics.median(r) - med) / med for r in rounds)
            res[k] = {'ms': round(med * 1e3, 4), 'spread': round(spread, 3), 'MB': round(nbytes[k] / 1e6, 1),
                      'GBs': round(nbytes[k] / med / 1e9, 1)}
        res['truth_over_covariance'] = round(res['truth_update']['ms'] / res['covariance_update']['ms'], 3)
        print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
