"""Restatement of the native-resolution warp in torch CPU calls at a given dtype, shared by the host and GPU tests: the
definition of DESIGN.md section 6 written out -- pad the native volume with the fill, resize the displacement from the
registration grid to the padded extent (trilinear, align_corners), grid_sample the padded volume at identity + displacement
(border, align_corners; trilinear for a float image, nearest for labels) and crop back to the native box.  Inputs are CPU
tensors; `dtype` is torch.float32 or torch.float64."""
import numpy as np
import torch
import torch.nn.functional as F

from ir_sgmcmc_amd.data_loader.synthetic import synthetic_pair
from ir_sgmcmc_amd.utils.imageio import write_nifti


def _pad_arg(grid):
    p = grid.padding
    return (p[2], p[2], p[1], p[1], p[0], p[0])


def _crop(t, grid):
    p, n = grid.padding, grid.shape
    return t[..., p[0]:p[0] + n[0], p[1]:p[1] + n[1], p[2]:p[2] + n[2]].contiguous()


def resized_displacement(u, grid, dtype):
    """u (C,3,*dims) -> (C,3,*padded) in `dtype`"""
    return F.interpolate(u.to(dtype), size=grid.padded, mode='trilinear', align_corners=True)


def identity(shape, dtype):
    """(1,3,*shape): channel 0 = linspace(-1, 1) along the last axis"""
    lin = [torch.linspace(-1, 1, n, dtype=dtype) for n in shape]
    z, y, x = torch.meshgrid(*lin, indexing='ij')
    return torch.stack((x, y, z)).unsqueeze(0)


def sample_grid(u, grid, dtype):
    """the grid_sample grid (C,*padded,3) in `dtype`"""
    return (identity(grid.padded, dtype) + resized_displacement(u, grid, dtype)).permute(0, 2, 3, 4, 1).contiguous()


def native_warp(u, grid, dtype, im=None, seg=None, mask=None, fill=None, scale=None):
    """-> dict with 'im' (C,1,*shape) in `dtype`, 'seg' int16, 'mask' bool and 'displacement' (C,3,*shape) in `dtype`, each when
    its input (`scale` for the displacement: three per-channel factors) is given.  im / seg / mask: (1 or C,1,*shape)."""
    C = u.shape[0]
    g = sample_grid(u, grid, dtype)
    out = {}
    if im is not None:
        padded = F.pad(im.to(dtype), _pad_arg(grid), value=float(im.min()) if fill is None else float(fill))
        out['im'] = _crop(F.grid_sample(padded.expand(C, -1, -1, -1, -1), g, mode='bilinear', padding_mode='border',
                                        align_corners=True), grid)
    for key, vol in (('seg', seg), ('mask', mask)):
        if vol is not None:
            padded = F.pad(vol.to(dtype), _pad_arg(grid), value=0.0)
            w = _crop(F.grid_sample(padded.expand(C, -1, -1, -1, -1), g, mode='nearest', padding_mode='border',
                                    align_corners=True), grid)
            out[key] = w.to(vol.dtype)
    if scale is not None:
        s = torch.tensor([float(x) for x in scale], dtype=dtype).view(1, 3, 1, 1, 1)
        out['displacement'] = _crop(resized_displacement(u, grid, dtype), grid) * s
    return out


def source_coordinate(u, grid):
    """the float64 source coordinate of every native voxel in padded index units, before the border clamp: (C,3,*shape) with
    entry a belonging to AXIS a of the native array (not to channel a)"""
    g = sample_grid(u, grid, torch.float64)  # (C,*padded,3), channel 0 = last axis
    P = torch.tensor([grid.padded[2], grid.padded[1], grid.padded[0]], dtype=torch.float64)
    q = (g + 1.0) / 2.0 * (P - 1.0)
    return _crop(q.permute(0, 4, 1, 2, 3).flip(1), grid)


def away_from_half(u, grid, margin=1e-3):
    """bool (C,1,*shape): the voxels whose clamped float64 source coordinate is farther than `margin` from a half-integer on
    all three axes -- where the nearest tap does not hang on the last bits of the coordinate"""
    q = source_coordinate(u, grid)
    last = torch.tensor([P - 1.0 for P in grid.padded], dtype=torch.float64).view(1, 3, 1, 1, 1)
    q = torch.minimum(torch.maximum(q, torch.zeros_like(q)), last)
    frac = q - torch.floor(q)
    return ((frac - 0.5).abs() > margin).all(dim=1, keepdim=True)


def smooth_field(C, dims, seed, amp=0.15):
    """a smooth random displacement (C,3,*dims) float32 in normalised units: amp * randn, box-filtered once (3^3, replicate)"""
    g = torch.Generator().manual_seed(seed)
    u = amp * torch.randn(C * 3, 1, *dims, generator=g)
    u = F.avg_pool3d(F.pad(u, (1, 1, 1, 1, 1, 1), mode='replicate'), 3, stride=1)
    return u.view(C, 3, *dims).contiguous()


def random_volumes(shape, seed, Cim=1):
    """native moving volumes (Cim,1,*shape): an image uniform in [0,1) float32, a segmentation of labels 0..5 in 2^3 blocks
    int16, and a bool mask"""
    g = torch.Generator().manual_seed(seed)
    im = torch.rand(Cim, 1, *shape, generator=g)
    coarse = torch.randint(0, 6, (Cim, 1, *[(n + 1) // 2 for n in shape]), generator=g)
    seg = coarse.repeat_interleave(2, 2).repeat_interleave(2, 3).repeat_interleave(2, 4)[..., :shape[0], :shape[1], :shape[2]]
    mask = torch.rand(Cim, 1, *shape, generator=g) > 0.3
    return im.contiguous(), seg.to(torch.int16).contiguous(), mask.contiguous()


def shifted(vol, grid, shift, fill):
    """`vol` (1,1,*shape) translated by integer voxels: out[i] = padded[clamp(i + p + shift, 0, P - 1)], the padded volume
    holding `fill` outside the native box -- what an integer source offset `shift` = (s0, s1, s2) per axis must give"""
    padded = F.pad(vol.double(), _pad_arg(grid), value=float(fill)).to(vol.dtype)  # exact for float32 / int16 / bool
    idx = [torch.clamp(torch.arange(n) + p + s, 0, P - 1) for n, p, s, P in zip(grid.shape, grid.padding, shift, grid.padded)]
    return padded[:, :, idx[0]][:, :, :, idx[1]][:, :, :, :, idx[2]].contiguous()


def constant_field(C, dims, per_channel):
    u = torch.zeros(C, 3, *dims)
    for c, v in enumerate(per_channel):
        u[:, c] = v
    return u


def write_pair(root, shape, zooms=(1.0, 1.5, 2.0), moving_shape=None):
    """two image / mask / seg triples of the synthetic generator under `root`, in the layout BiobankDataset reads"""
    for sub in ('', 'masks', 'segs'):
        (root / sub).mkdir(parents=True, exist_ok=True)
    vols = list(synthetic_pair(shape, seed=3))
    if moving_shape is not None:
        vols[1] = synthetic_pair(moving_shape, seed=3)[1]
    for i, vol in enumerate(vols):
        write_nifti(vol['im'][0].numpy(), str(root / f'im_{i}.nii.gz'), zooms)
        write_nifti(vol['mask'][0].numpy().astype(np.uint8), str(root / 'masks' / f'im_{i}.nii.gz'), zooms)
        write_nifti(vol['seg'][0].numpy(), str(root / 'segs' / f'im_{i}.nii.gz'), zooms)
    return str(root)
