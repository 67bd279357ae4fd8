"""Times the foreground-mask operators (ir_sgmcmc_amd/masks.py) on the synthetic fixed image.

Device events around every one of `--reps` calls after `--warmup` calls; the figure is the median.  One volume per size
(`--sizes`, default 128 256): the intensity histogram, the threshold, connected components at 26 and at 6, keep_largest,
fill_holes, dilate / erode / close at radius 2 and dilate at radius 8 and 16 on the thresholded image, and the whole
`foreground_mask` pipeline (wall time around a synchronised call: it reads the histogram and the counts back).  With
`--host` the same steps with scipy.ndimage on the host of the same box, wall time, for scale.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps, warmup):
    """median milliseconds per call, by device events"""
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    torch.cuda.synchronize()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return round(statistics.median(a.elapsed_time(b) for a, b in ev), 4)


def wall(fn, reps):
    """median milliseconds per call, host clock around a synchronised call"""
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        start = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - start) * 1e3)
    return round(statistics.median(out), 3)


def host_steps(im, threshold):
    """the pipeline with scipy.ndimage, step by step -> {step: milliseconds}"""
    from scipy import ndimage
    res = {}

    def step(name, fn):
        start = time.perf_counter()
        out = fn()
        res[name] = round((time.perf_counter() - start) * 1e3, 1)
        return out

    def ball(radius):
        r = int(radius)
        z, y, x = np.ogrid[-r:r + 1, -r:r + 1, -r:r + 1]
        return z * z + y * y + x * x <= radius * radius

    mask = step('threshold', lambda: im > threshold)
    labels, n = step('label_26', lambda: ndimage.label(mask, np.ones((3, 3, 3))))
    mask = step('keep_largest', lambda: labels == 1 + int(np.argmax(np.bincount(labels.ravel())[1:])))
    mask = step('fill_holes', lambda: ndimage.binary_fill_holes(mask))
    mask = step('close_r2', lambda: ndimage.binary_erosion(ndimage.binary_dilation(mask, ball(2)), ball(2), border_value=1))
    step('dilate_r1', lambda: ndimage.binary_dilation(mask, ball(1)))
    step('dilate_r8_by_edt', lambda: ndimage.distance_transform_edt(~mask) <= 8)
    res['pipeline'] = round(sum(res.values()) - res['dilate_r8_by_edt'], 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--sizes', type=int, nargs='+', default=[128, 256])
    ap.add_argument('--host', action='store_true', help='also time scipy.ndimage on the host')
    args = ap.parse_args()
    from ir_sgmcmc_amd import masks as M
    from ir_sgmcmc_amd.data_loader import synthetic_pair
    dev = 'cuda:0'
    res = {'reps': args.reps, 'warmup': args.warmup}
    for n in args.sizes:
        fixed, _ = synthetic_pair((n, n, n), seed=0)
        im = fixed['im'].unsqueeze(0).to(dev)
        value_range = tuple(float(x) for x in (im.min(), im.max()))
        mask, summary = M.foreground_mask(im, closing=2, dilation=1)
        raw = M.threshold_mask(im, summary['threshold'])
        t = lambda fn: timed(fn, args.reps, args.warmup)
        row = {'voxels': summary['voxels'], 'components': summary['components'], 'threshold': round(summary['threshold'], 5),
               'histogram_256_ms': t(lambda: M.intensity_histogram(im, 256, value_range)),
               'threshold_ms': t(lambda: M.threshold_mask(im, summary['threshold'])),
               'components_26_ms': t(lambda: M.connected_components(raw, 26)),
               'components_6_ms': t(lambda: M.connected_components(raw, 6)),
               'keep_largest_ms': t(lambda: M.keep_largest(raw, 26, 1)),
               'fill_holes_ms': t(lambda: M.fill_holes(mask)),
               'dilate_r2_ms': t(lambda: M.dilate(mask, 2)), 'erode_r2_ms': t(lambda: M.erode(mask, 2)),
               'close_r2_ms': t(lambda: M.close(mask, 2)), 'dilate_r8_ms': t(lambda: M.dilate(mask, 8)),
               'dilate_r16_ms': t(lambda: M.dilate(mask, 16)),
               'pipeline_wall_ms': wall(lambda: M.foreground_mask(im, closing=2, dilation=1), args.reps)}
        if args.host:
            row['host_scipy_ms'] = host_steps(fixed['im'][0].numpy(), np.float32(summary['threshold']))
        res[f'{n}^3'] = row
    print(json.dumps(res))


if __name__ == '__main__':
    main()
