"""Times ops.image_similarity (joint histogram + moment sums in one pass, then entropies / MI / NMI / MSE / NCC) against a
device-to-device copy and against the torch composition a user would write for the same ten numbers: two bin-index volumes, an
int64 combined index, a bincount and the moment reductions.

Ranges given (no host read-back in the operator), want_hist off, 64 bins, mask on (a ball, as a brain mask is a blob), at 256^3
with one chain and at 128^3 with two, on three kinds of image pair:
  constant  every voxel in ONE joint bin -- the worst case for same-address LDS adds;
  smooth    a 12^3 grid of uniform draws interpolated trilinearly, moving = 0.7 fixed + 0.3 another such field -- what a real
            image looks like to the histogram (neighbours share their bin); the product's case;
  random    uniform white noise, moving = 0.7 fixed + 0.3 noise -- neighbours never share a bin.
The operator is timed once per value of the switch `similarity_aggregate` in --aggregate (0: plain LDS atomics always; 1: a
wavefront whose voxels all fall into one joint bin adds their number with one LDS add).

Device events around every one of `--reps` calls after `--warmup` calls; the figure is the median.  The paths are alternated,
twice, and the better median of each is kept: other work shares the device.  The timed buffers are cache-resident: the calls
repeat on the same 151 MB (256^3) / 84 MB (128^3, two chains), less than the 256 MB last-level cache.  Bytes are what the
algorithm must move: 9 per voxel and chain (fixed 4, moving 4, mask 1; the shared fixed image and mask are counted per chain, as
the kernel reads them).  The copy rate is a torch copy_ of a 2 GiB buffer, counted as read + write.  Peak memory is torch's
allocator peak above the inputs during one call.  One JSON line per size and image kind, printed and written to --out.  Run it
under `rocprofv3 --kernel-trace --stats` with `--no-baseline` for the kernel times alone.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ir_sgmcmc_amd import _lib as L  # noqa: E402
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


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def smooth_field(C, dims, gen, dev):
    low = torch.rand(C, 1, 12, 12, 12, device=dev, generator=gen)
    return F.interpolate(low, size=dims, mode='trilinear', align_corners=True).contiguous()


def make_pair(kind, C, dims, gen, dev):
    if kind == 'constant':
        return torch.full((1, 1, *dims), 0.5, device=dev), torch.full((C, 1, *dims), 0.25, device=dev)
    draw = smooth_field if kind == 'smooth' else (lambda c, d, g, dv: torch.rand(c, 1, *d, device=dv, generator=g))
    fixed = draw(1, dims, gen, dev)
    return fixed, (0.7 * fixed + 0.3 * draw(C, dims, gen, dev)).contiguous()


def ball_mask(dims, dev):
    ax = [torch.linspace(-1, 1, n, device=dev) for n in dims]
    z, y, x = torch.meshgrid(*ax, indexing='ij')
    return (z * z + y * y + x * x < 0.9)[None, None].contiguous()


def composition(fixed, moving, mask, bins, lo=0.0, hi=1.0):
    """the same ten numbers per chain, composed in torch on the device"""
    inv = bins / (hi - lo)
    inside = mask.reshape(-1)
    rows = []
    for c in range(moving.shape[0]):
        f, m = fixed[0].reshape(-1), moving[c].reshape(-1)
        finite = torch.isfinite(f) & torch.isfinite(m)
        take = inside & finite
        bf = ((f - lo) * inv).floor().clamp(0, bins - 1).long()       # bin-index volume of the fixed image
        bm = ((m - lo) * inv).floor().clamp(0, bins - 1).long()       # ... of the moving image
        idx = torch.where(take, bf * bins + bm, 0)                    # the int64 combined index
        w = take.double()
        hist = torch.bincount(idx, weights=w, minlength=bins * bins).view(bins, bins)
        n = w.sum()
        fd, md = torch.where(take, f, 0.0).double(), torch.where(take, m, 0.0).double()
        s_d2, s_f, s_m = ((fd - md) ** 2).sum(), fd.sum(), md.sum()
        s_ff, s_mm, s_fm = (fd * fd).sum(), (md * md).sum(), (fd * md).sum()
        clipped = (take & ((f < lo) | (f > hi) | (m < lo) | (m > hi))).sum()

        def entropy(counts):
            p = counts.reshape(-1) / n
            return -(torch.where(p > 0, p * torch.log(p), 0.0)).sum()
        hf, hm, hj = entropy(hist.sum(1)), entropy(hist.sum(0)), entropy(hist)
        mf, mm = s_f / n, s_m / n
        ncc = (s_fm / n - mf * mm) / torch.sqrt((s_ff / n - mf * mf) * (s_mm / n - mm * mm))
        rows.append(torch.stack([n, (inside & ~finite).sum().double(), clipped.double(), s_d2 / n, ncc, hf, hm, hj, hf + hm - hj,
                                 (hf + hm) / hj]))
    return torch.stack(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--bins', type=int, default=64)
    ap.add_argument('--aggregate', type=int, nargs='+', default=[0, 1], help='values of similarity_aggregate to time')
    ap.add_argument('--default-aggregate', type=int, default=1, help='the value the switch is left at')
    ap.add_argument('--no-baseline', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'image_similarity_bench.txt'))
    args = ap.parse_args()
    dev = 'cuda:0'
    src = torch.empty(1 << 29, device=dev)  # 2 GiB
    dst = torch.empty_like(src)
    t_copy = timed(lambda: dst.copy_(src), args.reps, args.warmup)
    copy_gbs = 2 * src.numel() * 4 / t_copy / 1e9
    del src, dst

    lines = []
    gen = torch.Generator(device=dev).manual_seed(0)
    for C, dims in ((1, (256, 256, 256)), (2, (128, 128, 128))):
        mask = ball_mask(dims, dev)
        for kind in ('constant', 'smooth', 'random'):
            fixed, moving = make_pair(kind, C, dims, gen, dev)

            def hip():
                return ops.image_similarity(fixed, moving, mask, args.bins, (0.0, 1.0), (0.0, 1.0))['stats']

            def torch_path():
                return composition(fixed, moving, mask, args.bins)

            paths = {}
            for r in args.aggregate:
                paths[f'hip_aggregate_{r}'] = (lambda r=r: (L.option_set('similarity_aggregate', r), hip())[1])
            if not args.no_baseline:
                paths['torch_composition'] = torch_path
                a, b = hip(), torch_path()
                ok = ~torch.isnan(b)
                agree = float(((a - b).abs() / b.abs().clamp(min=1.0))[ok].max())
                same_nan = bool((torch.isnan(a) == torch.isnan(b)).all())
                del a, b
            best = {k: [] for k in paths}
            for _ in range(2):
                for k, fn in paths.items():
                    best[k].append(timed(fn, args.reps, args.warmup))
            best = {k: min(v) for k, v in best.items()}
            L.option_set('similarity_aggregate', args.default_aggregate)
            V = dims[0] * dims[1] * dims[2]
            moved = 9 * V * C
            line = {'dims': list(dims), 'chains': C, 'bins': args.bins, 'image': kind, 'copy_GBs': round(copy_gbs, 1),
                    'moved_MB': round(moved / 1e6, 1)}
            for r in args.aggregate:
                t = best[f'hip_aggregate_{r}']
                line[f'hip_aggregate_{r}_us'] = round(t * 1e6, 1)
                line[f'hip_aggregate_{r}_fraction_of_copy'] = round(moved / t / 1e9 / copy_gbs, 3)
            line['hip_peak_MB'] = round(peak_bytes(hip) / 1e6, 2)
            if not args.no_baseline:
                line['torch_composition_us'] = round(best['torch_composition'] * 1e6, 1)
                line['torch_composition_peak_MB'] = round(peak_bytes(torch_path) / 1e6, 1)
                line['torch_over_hip_default'] = round(best['torch_composition'] / best[f'hip_aggregate_{args.default_aggregate}'], 2) \
                    if args.default_aggregate in args.aggregate else None
                line['stats_max_rel_diff'] = agree
                line['nan_pattern_agrees'] = same_nan
            print(json.dumps(line), flush=True)
            lines.append(json.dumps(line))
            del fixed, moving
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
