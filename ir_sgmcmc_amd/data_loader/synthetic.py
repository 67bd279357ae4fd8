"""Deterministic synthetic fixed/moving pair.

The reference ships no image data (`configs/*/config.json:92` point at the author's cluster), so the
bench, the smoke test and the parity tests use this generator.  It yields the same dict contract as
the reference's `BiobankDataset.__getitem__` (data_loader/datasets.py:107-145): `fixed`/`moving` dicts
with `im` float32 (1,D,H,W), `mask` bool, `seg` int16, plus the VI parameters `mu`, `log_var`, `u`.
Host-side, CPU tensors; the trainer moves them to the device.
"""
import math

import torch


def _coords(dims):
    D, H, W = dims
    z = torch.linspace(-1, 1, D).view(D, 1, 1)
    y = torch.linspace(-1, 1, H).view(1, H, 1)
    x = torch.linspace(-1, 1, W).view(1, 1, W)
    return z, y, x


def _blobs(dims, shift_a, shift_b):
    z, y, x = _coords(dims)
    za, ya, xa = shift_a
    r2 = (z - za) ** 2 + (y - ya) ** 2 + (x - xa) ** 2
    zb, yb, xb = 0.3 + shift_b[0], -0.2 + shift_b[1], 0.1 + shift_b[2]
    q2 = (z - zb) ** 2 + (y - yb) ** 2 + (x - xb) ** 2
    return torch.exp(-4.0 * r2) + 0.5 * torch.exp(-30.0 * q2)


def misalign_triple(triple, rotation_deg, shift):
    """{'im', 'mask', 'seg'} of (1,D,H,W) read at p = c + shift + R (k - c) on the host: R the rotation about the vector
    `rotation_deg` (array order, its length the angle in degrees), `shift` in voxels, c the centre of the grid.  Trilinear for
    the image, nearest for mask and segmentation, border padding.  The pair a pre-alignment (trainer.affine_init) has to undo."""
    import torch.nn.functional as F
    D, H, W = triple['im'].shape[1:]
    w = torch.tensor([math.radians(float(a)) for a in rotation_deg], dtype=torch.float64)
    angle = float(w.norm())
    K = torch.zeros(3, 3, dtype=torch.float64)
    if angle > 0:
        a0, a1, a2 = (w / angle).tolist()
        K = torch.tensor([[0.0, -a2, a1], [a2, 0.0, -a0], [-a1, a0, 0.0]], dtype=torch.float64)
    R = torch.eye(3, dtype=torch.float64) + math.sin(angle) * K + (1.0 - math.cos(angle)) * (K @ K)
    c = torch.tensor([(D - 1) / 2.0, (H - 1) / 2.0, (W - 1) / 2.0], dtype=torch.float64)
    k = torch.stack(torch.meshgrid(*[torch.arange(n, dtype=torch.float64) for n in (D, H, W)], indexing='ij'), -1)
    p = (k - c) @ R.T + c + torch.tensor([float(s) for s in shift], dtype=torch.float64)
    grid = (p / c - 1.0).flip(-1).float().unsqueeze(0)  # [-1, 1], x first
    sample = lambda vol, mode: F.grid_sample(vol.float().unsqueeze(0), grid, mode=mode, padding_mode='border', align_corners=True)[0]
    return {'im': sample(triple['im'], 'bilinear').contiguous(), 'mask': sample(triple['mask'], 'nearest').bool().contiguous(),
            'seg': sample(triple['seg'], 'nearest').to(torch.int16).contiguous()}


MOVING_CONTRASTS = ('invert', 'fold')


def moving_contrast_map(im, kind):
    """another contrast for the moving image, the anatomy unchanged: "invert" m <- max + min - m (a monotone decreasing map: T1 / T2
    like), "fold" m <- 4 s (1 - s) of the image rescaled to s in [0, 1] (non-monotone: two intensities of the fixed image share one
    of the moving image)"""
    if kind not in MOVING_CONTRASTS:
        raise ValueError(f'moving_contrast {kind!r}: null or one of {list(MOVING_CONTRASTS)}')
    lo, hi = im.min(), im.max()
    if kind == 'invert':
        return hi + lo - im
    s = (im - lo) / (hi - lo)
    return 4.0 * s * (1.0 - s)


def moving_bias_field(im, a):
    """a smooth intensity inhomogeneity for the moving image (bias field, coil shading): m <- m exp(a z_n), z_n the normalised
    first coordinate in [-1, 1]"""
    if isinstance(a, bool) or not isinstance(a, (int, float)) or not math.isfinite(a):
        raise ValueError(f'moving_bias {a!r}: null or a finite number')
    z, _, _ = _coords(tuple(im.shape))
    return im * torch.exp(float(a) * z)


def synthetic_pair(dims, seed=0, noise=0.02, misalign=None, moving_contrast=None, moving_bias=None):
    """Two Gaussian blobs + white noise; the moving image has both blobs shifted.  Returns (fixed, moving).
    misalign: None (the pair as it always was), or {"rotation_deg": [a0, a1, a2], "shift": [s0, s1, s2]}: the moving triple
    is then rotated and shifted on the host (misalign_triple).
    moving_contrast: None (the pair as it always was), "invert" or "fold" (moving_contrast_map): the moving image in another
    contrast, which only a mutual-information data term registers.
    moving_bias: None (the pair as it always was), or a number a: the moving image is then multiplied by exp(a z_n) after
    moving_contrast (moving_bias_field), an inhomogeneity that spreads one tissue over many bins of a global histogram."""
    dims = tuple(int(d) for d in dims)
    g = torch.Generator().manual_seed(seed)
    im_f = _blobs(dims, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)) + noise * torch.randn(dims, generator=g)
    im_m = _blobs(dims, (0.08, -0.04, 0.05), (0.06, 0.05, 0.02)) + noise * torch.randn(dims, generator=g)
    if moving_contrast is not None:
        im_m = moving_contrast_map(im_m, moving_contrast)
    if moving_bias is not None:
        im_m = moving_bias_field(im_m, moving_bias)
    z, y, x = _coords(dims)
    r2 = z ** 2 + y ** 2 + x ** 2
    mask = (r2 < 0.9).expand(dims)
    # three nested label shells so that nearest-neighbour warps / Dice have something to chew on
    seg = (torch.zeros(dims, dtype=torch.int16) + (r2 < 0.5).to(torch.int16) * 10 + (r2 < 0.2).to(torch.int16) * 6
           + (r2 < 0.05).to(torch.int16) * 33)

    def pack(im):
        return {'im': im.float().unsqueeze(0).contiguous(), 'mask': mask.unsqueeze(0).contiguous(),
                'seg': seg.unsqueeze(0).contiguous()}

    fixed, moving = pack(im_f), pack(im_m)
    if misalign is not None:
        unknown = set(misalign) - {'rotation_deg', 'shift'}
        if unknown:
            raise ValueError(f'misalign: unknown keys {sorted(unknown)}; known: ["rotation_deg", "shift"]')
        moving = misalign_triple(moving, misalign.get('rotation_deg', (0.0, 0.0, 0.0)), misalign.get('shift', (0.0, 0.0, 0.0)))
    return fixed, moving


FIXED_BLOBS = ((0.0, 0.0, 0.0), (0.3, -0.2, 0.1))          # the centres _blobs is called with above, normalised (z, y, x)
MOVING_BLOBS = ((0.08, -0.04, 0.05), (0.36, -0.15, 0.12))


def synthetic_landmarks(dims):
    """The two blob centres of synthetic_pair as corresponding landmarks -> (fixed, moving), each a (2,3) float64 array of
    registration-grid voxel indices in (D,H,W) order: ((g + 1) / 2) * (n - 1) of the normalised centres, not rounded."""
    import numpy as np
    nm1 = np.asarray([int(d) - 1 for d in dims], dtype=np.float64)
    to_index = lambda blobs: (np.asarray(blobs, dtype=np.float64) + 1.0) / 2.0 * nm1
    return to_index(FIXED_BLOBS), to_index(MOVING_BLOBS)


def init_var_params(dims_v, sigma_v_init=0.5, u_v_init=0.1):
    """mu = 0, log_var = log(sigma^2), u = const (data_loader/datasets.py:57-68)."""
    shape = (3, *dims_v)
    return {'mu': torch.zeros(shape), 'log_var': torch.full(shape, math.log(sigma_v_init ** 2)),
            'u': torch.full(shape, float(u_v_init))}
