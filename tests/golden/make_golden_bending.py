#!/usr/bin/env python3
"""Fixture of the bending energy: the reference's own `GradientOperator` (utils/diff_op.py:62-96) applied twice, in float64.

    n1 = G(v)                          (C, 3[axis], D, H, W, 3[comp])
    H_comp = G(n1[..., comp])          (C, 3[a], D, H, W, 3[b]) = d_a d_b v_comp
    y_c = sum over comp, a, b, voxels of H_comp^2

and dy/dv by autograd through that composition.  Seeded normal fields at (C,3,D,H,W) = (2,3,3,3,3), (1,3,2,5,6), (2,3,7,9,11).
Output: tests/golden/bending_ops.npz with v_i, y_i, g_i per case (float64 data, no reference source).  Runs only where the
reference tree is at hand.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_bending.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from _ref_import import import_reference  # noqa: E402

SHAPES = [(2, 3, 3, 3, 3), (1, 3, 2, 5, 6), (2, 3, 7, 9, 11)]


def main():
    ref = import_reference()
    G = ref.utils.GradientOperator()
    out = {}
    for i, shape in enumerate(SHAPES):
        v = torch.randn(shape, dtype=torch.float64, generator=torch.Generator().manual_seed(1234 + i)).requires_grad_(True)
        n1 = G(v)
        y = sum((G(n1[..., comp]) ** 2).sum(dim=(1, 2, 3, 4, 5)) for comp in range(3))
        g, = torch.autograd.grad(y.sum(), v)
        out[f'v_{i}'], out[f'y_{i}'], out[f'g_{i}'] = v.detach().numpy(), y.detach().numpy(), g.numpy()
    np.savez_compressed(os.path.join(HERE, 'bending_ops.npz'), **out)
    print({k: a.shape for k, a in out.items()})


if __name__ == '__main__':
    main()
