"""Timings of the MI data term's three kernels (csrc/mi_kernels.hip) through the stateless operators.

    python tools/mi_bench.py --size 256 --chains 1 --bins 32 --image pair --calls 20

runs `calls` pairs of mi_forward (memset + accumulate + finish) and mi_backward (gradient, with the pmi map when --pmi) on the
synthetic pair with the moving image inverted (`--image pair`) or on a constant moving image (`--image constant`: every wavefront
hits the same four cells of the histogram) and prints one JSON line with the HIP-event time per call of each.  Run it under
`rocprofv3 --kernel-trace --stats` for the kernel times alone.  `--all` walks sizes, bins and images in one process (HIP events
only: the kernels of all configurations share their names)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ir_sgmcmc_amd import mi  # noqa: E402
from ir_sgmcmc_amd.data_loader import synthetic_pair  # noqa: E402

DEV = 'cuda:0'


def inputs(size, chains, image):
    f, m = synthetic_pair((size,) * 3, seed=0, moving_contrast='invert')
    fixed, mask = f['im'].unsqueeze(0).to(DEV), f['mask'].unsqueeze(0).to(DEV)
    moving = m['im'].unsqueeze(0).to(DEV).repeat(chains, 1, 1, 1, 1).contiguous()
    if image == 'constant':
        moving.fill_(0.5)
    return fixed, moving, mask


def run(size, chains, bins, image, calls, pmi=False):
    fixed, moving, mask = inputs(size, chains, image)
    f_range, m_range = mi.mi_ranges(fixed, moving, mask)
    if image == 'constant':
        m_range = (0.0, 1.0)
    out = mi.mi_forward(fixed, moving, mask, bins, f_range, m_range)
    mi.mi_backward(fixed, moving, out['table'], mask, bins, f_range, m_range, want_pmi=pmi)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(calls):
        out = mi.mi_forward(fixed, moving, mask, bins, f_range, m_range)
    ev[1].record()
    for _ in range(calls):
        mi.mi_backward(fixed, moving, out['table'], mask, bins, f_range, m_range, want_pmi=pmi)
    ev[2].record()
    torch.cuda.synchronize()
    n = float(out['stats'][0, 0])
    return {'size': size, 'chains': chains, 'bins': bins, 'image': image, 'pmi': pmi, 'n': n,
            'mi': float(out['stats'][0, 3]), 'fwd_us': 1e3 * ev[0].elapsed_time(ev[1]) / calls,
            'bwd_us': 1e3 * ev[1].elapsed_time(ev[2]) / calls}


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--size', type=int, default=256)
    p.add_argument('--chains', type=int, default=1)
    p.add_argument('--bins', type=int, default=32)
    p.add_argument('--image', choices=('pair', 'constant'), default='pair')
    p.add_argument('--calls', type=int, default=20)
    p.add_argument('--pmi', action='store_true')
    p.add_argument('--all', action='store_true')
    a = p.parse_args()
    if not a.all:
        print(json.dumps(run(a.size, a.chains, a.bins, a.image, a.calls, a.pmi)))
        return
    for size, chains in ((256, 1), (128, 2)):
        for bins in (32, 64):
            for image in ('pair', 'constant'):
                print(json.dumps(run(size, chains, bins, image, a.calls)), flush=True)


if __name__ == '__main__':
    main()
