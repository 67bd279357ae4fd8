"""Times the posterior-mode kernels (modes.modes_append: irs_modes_gram_rows behind the copy of the new records; modes.modes_project:
irs_modes_project) against a device-to-device copy and against the torch compositions they replace.

Device events around every one of `--reps` calls after `--warmup` calls; the figure is the median.  The store holds white noise
on a smooth offset.  Bytes are what the algorithm must move.  Gram rows: the n = n_before + n_new stored records once (12 V n),
the n_new new records again for every tile of 8 stored records at or below the diagonal (12 V n_new ceil(n / 8)) and the mask
(V).  Projection: the n records once (12 V n) and the outputs (12 V + 12 V M + 4 V).  The copy rate is a torch copy_ of a 2 GiB
buffer, counted as read + write.  The torch composition of the Gram rows: the store slice and the new records cast to float64,
masked, one batched matmul per call; of the projection: a float64 matmul of the coefficients with the cast store, the mean and
the elementwise variance.  Prints one JSON line per measurement.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ir_sgmcmc_amd import modes  # noqa: E402


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
    ap.add_argument('--cap', type=int, default=256)
    ap.add_argument('--before', type=int, nargs='+', default=[0, 64, 254])
    ap.add_argument('--modes', type=int, default=8)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--baseline-bytes', type=float, default=60e9, help='largest float64 copy of the store the torch baseline may make')
    args = ap.parse_args()
    dev = 'cuda:0'
    src = torch.empty(1 << 29, device=dev)  # 2 GiB
    dst = torch.empty_like(src)
    copy_gbs = 2 * src.numel() * 4 / timed(lambda: dst.copy_(src), args.reps, args.warmup) / 1e9
    del src, dst
    C, cap, M = args.chains, args.cap, args.modes
    for size in args.sizes:
        V = size ** 3
        g = torch.Generator(device=dev).manual_seed(0)
        mask = torch.rand(size, size, size, device=dev, generator=g) < 0.6
        st = modes.modes_state((size,) * 3, cap, dev, mask)
        offset = 0.05 * torch.randn(1, 3, size, size, size, device=dev, generator=g)
        for i in range(0, cap, 8):  # filled in pieces: no second copy of the store
            st['store'][i:i + 8] = offset + 0.01 * torch.randn(min(8, cap - i), 3, size, size, size, device=dev, generator=g)
        new = st['store'][:C].clone()
        for n_before in args.before:
            n = n_before + C
            if n > cap:
                continue

            def append():
                st['n'] = n_before
                modes.modes_append(st, new)

            t = timed(append, args.reps, args.warmup)
            nbytes = 12 * V * n + 12 * V * C * ((n + 7) // 8) + V
            out = {'kernel': 'gram_rows', 'size': size, 'chains': C, 'n_before': n_before, 'copy_GBs': round(copy_gbs, 1),
                   'ms': round(t * 1e3, 4), 'MB': round(nbytes / 1e6, 1), 'GBs': round(nbytes / t / 1e9, 1),
                   'over_copy_rate': round(nbytes / t / 1e9 / copy_gbs, 3)}
            if 24.0 * V * n <= args.baseline_bytes:
                gram_b = torch.zeros(3, cap, cap, device=dev, dtype=torch.float64)
                m64 = mask.reshape(1, 1, V).double()

                def baseline():
                    st['store'][n_before:n] = new
                    x = st['store'][:n].reshape(n, 3, V).double() * m64
                    rows = torch.matmul(x[n_before:].permute(1, 0, 2), x.permute(1, 2, 0))  # (3, C, n)
                    gram_b[:, n_before:n, :n] = rows
                    gram_b[:, :n, n_before:n] = rows.transpose(1, 2)

                tb = timed(baseline, max(args.reps // 4, 3), 1)
                out.update({'baseline_ms': round(tb * 1e3, 4), 'baseline_over_kernel': round(tb / t, 2)})
                del gram_b, m64
            print(json.dumps(out), flush=True)
        st['n'] = cap
        coeff = torch.randn(M, cap, device=dev, dtype=torch.float64, generator=g) / cap
        scale = ((size - 1) / 2,) * 3
        t = timed(lambda: modes.modes_project(st, coeff, scale), max(args.reps // 2, 3), 2)
        nbytes = 12 * V * cap + (12 + 12 * M + 4) * V
        out = {'kernel': 'project', 'size': size, 'n': cap, 'modes': M, 'copy_GBs': round(copy_gbs, 1), 'ms': round(t * 1e3, 4),
               'MB': round(nbytes / 1e6, 1), 'GBs': round(nbytes / t / 1e9, 1), 'over_copy_rate': round(nbytes / t / 1e9 / copy_gbs, 3)}
        if 24.0 * V * cap <= args.baseline_bytes:
            s2 = torch.tensor([s * s for s in scale], device=dev, dtype=torch.float64).reshape(3, 1)

            def baseline():
                x = st['store'].reshape(cap, 3 * V).double()
                fields = torch.matmul(coeff, x).reshape(M, 3, V)
                mean = x.mean(dim=0)
                var = x.var(dim=0).reshape(3, V)
                return mean.float(), fields.float(), ((s2 * (fields ** 2).sum(dim=0)).sum(dim=0) / (s2 * var).sum(dim=0)).float()

            tb = timed(baseline, 3, 1)
            out.update({'baseline_ms': round(tb * 1e3, 4), 'baseline_over_kernel': round(tb / t, 2)})
        print(json.dumps(out), flush=True)
        del st, new, offset, mask


if __name__ == '__main__':
    main()
