"""Times ops.native_warp (the fused upsample-and-warp onto the image's own voxel grid) against a device-to-device copy and
against the torch composition a user would write for the same outputs: resize the displacement to the padded extent, add the
identity, pad the native image and segmentation, grid_sample both (trilinear / nearest) and crop.

Device events around every one of `--reps` calls after `--warmup` calls; the figure is the median.  One chain, image +
segmentation in one launch.  The field is smooth random (a 4^3 grid of normal draws, trilinearly upsampled, about +-3 native
voxels), the image uniform random, the segmentation 4^3 blocks of eight labels.  Bytes are what the algorithm must move: every
native voxel of the image (4 B) and of the segmentation (2 B) read once, the three channels of the field read once (12 B per
grid voxel), the two outputs written (4 + 2 B).  The copy rate is a torch copy_ of a 2 GiB buffer, counted as read + write.
Peak memory is torch's allocator peak above the inputs during one call.  Prints one JSON line.  Run it under
`rocprofv3 --kernel-trace --stats` for the kernel time alone.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ir_sgmcmc_amd import ops  # noqa: E402
from ir_sgmcmc_amd.native import NativeGrid  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--native', type=int, nargs=3, default=[182, 218, 182])
    ap.add_argument('--dims', type=int, nargs=3, default=[128, 128, 128])
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    dev = 'cuda:0'
    src = torch.empty(1 << 29, device=dev)  # 2 GiB
    dst = torch.empty_like(src)
    t_copy = timed(lambda: dst.copy_(src), args.reps, args.warmup)
    copy_gbs = 2 * src.numel() * 4 / t_copy / 1e9
    del src, dst

    grid = NativeGrid.from_shape(args.native, args.dims)
    n, p, P, m = grid.shape, grid.padding, grid.padded, grid.dims
    g = torch.Generator(device=dev).manual_seed(0)
    u = F.interpolate(torch.randn(1, 3, 4, 4, 4, device=dev, generator=g) * 0.012, size=m, mode='trilinear',
                      align_corners=True).contiguous()
    im = torch.rand(1, 1, *n, device=dev, generator=g)
    blocks = torch.randint(0, 8, (1, 1, *[(k + 3) // 4 for k in n]), device=dev, generator=g)
    seg = blocks.repeat_interleave(4, 2).repeat_interleave(4, 3).repeat_interleave(4, 4)[..., :n[0], :n[1], :n[2]]
    seg = seg.to(torch.int16).contiguous()
    fill = float(im.min())
    pad = (p[2], p[2], p[1], p[1], p[0], p[0])
    lin = [torch.linspace(-1.0, 1.0, k, device=dev) for k in P]
    identity = torch.stack(torch.meshgrid(*lin, indexing='ij')).flip(0).permute(1, 2, 3, 0)[None].contiguous()  # kept: not timed

    def crop(t):
        return t[..., p[0]:p[0] + n[0], p[1]:p[1] + n[1], p[2]:p[2] + n[2]].contiguous()

    def hip():
        return ops.native_warp(u, grid, im=im, seg=seg, fill=fill)

    def composition():
        field = F.interpolate(u, size=P, mode='trilinear', align_corners=True)
        sample_at = identity + field.permute(0, 2, 3, 4, 1)
        im_w = F.grid_sample(F.pad(im, pad, value=fill), sample_at, mode='bilinear', padding_mode='border', align_corners=True)
        seg_w = F.grid_sample(F.pad(seg.float(), pad), sample_at, mode='nearest', padding_mode='border', align_corners=True)
        return {'im': crop(im_w), 'seg': crop(seg_w).to(torch.int16)}

    a, b = hip(), composition()
    seg_differs = float((a['seg'] != b['seg']).float().mean())
    im_diff = float((a['im'] - b['im']).abs().max())
    del a, b
    # alternate the two, twice, and keep the better median of each: other work shares the device
    t_hip, t_torch = [], []
    for _ in range(2):
        t_hip.append(timed(hip, args.reps, args.warmup))
        t_torch.append(timed(composition, args.reps, args.warmup))
    t_hip, t_torch = min(t_hip), min(t_torch)
    V, Vm = n[0] * n[1] * n[2], m[0] * m[1] * m[2]
    moved = V * (4 + 2 + 4 + 2) + 12 * Vm
    print(json.dumps({'native': list(n), 'padded': list(P), 'dims': list(m), 'copy_GBs': round(copy_gbs, 1),
                      'native_warp_ms': round(t_hip * 1e3, 4), 'moved_MB': round(moved / 1e6, 1),
                      'native_warp_GBs': round(moved / t_hip / 1e9, 1), 'fraction_of_copy': round(moved / t_hip / 1e9 / copy_gbs, 3),
                      'torch_composition_ms': round(t_torch * 1e3, 4), 'torch_over_native_warp': round(t_torch / t_hip, 2),
                      'native_warp_peak_MB': round(peak_bytes(hip) / 1e6, 1),
                      'torch_composition_peak_MB': round(peak_bytes(composition) / 1e6, 1),
                      'displacement_max_voxels': round(float(u.abs().max()) * (max(P) - 1) / 2, 2),
                      'im_max_abs_diff': im_diff, 'seg_fraction_differing': seg_differs}), flush=True)


if __name__ == '__main__':
    main()
