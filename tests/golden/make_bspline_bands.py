"""Writes tests/golden/bspline_bands.json: per native case of tests/_bspline.py the largest deviation of the float32 restatement
(the device's operation order) from the float64 one over the cubic voxels, on the CPU, and four times that as the band
irs_native_warp_cubic is held to.  Run from the repository root: python tests/golden/make_bspline_bands.py"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import _bspline as B  # noqa: E402

FACTOR = 4

if __name__ == '__main__':
    cases = {}
    for shape, dims in B.NATIVE_CASES:
        worst = 0.0
        for seed in B.NATIVE_SEEDS:
            grid, u, im, fill = B.native_inputs(shape, dims, seed)
            coeff = torch.from_numpy(B.prefilter(im.numpy()))
            r64, r32 = B.native_float64(u, grid, im, coeff, fill), B.native_float32(u, grid, coeff)
            both = ~r64['near_face'] & r64['cubic'] & r32['cubic']
            worst = max(worst, float(np.abs(r32['value'].astype(np.float64) - r64['value'])[both].max()))
        cases['x'.join(map(str, shape))] = {'measured': worst, 'band': FACTOR * worst}
    about = ('largest |float32 restatement - float64 restatement| over the cubic voxels of the native cases of tests/_bspline.py '
             '(seeds 1 and 2, C = 2), measured on the CPU, and the band the GPU test holds irs_native_warp_cubic to: 4 x measured')
    with open(os.path.join(ROOT, 'tests', 'golden', 'bspline_bands.json'), 'w') as f:
        json.dump({'note': about, 'factor': FACTOR, 'cases': cases}, f, indent=1)
