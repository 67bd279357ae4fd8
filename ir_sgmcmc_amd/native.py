"""Geometry of the image's own voxel grid against the registration grid (host only; absent in the reference, whose outputs all
live on the registration grid).

BiobankDataset pads a native volume of shape n = (n0, n1, n2) -- treated as (D, H, W), as `read_nifti` returns it -- with
p_a = (max(n) - n_a) // 2 voxels on both sides of axis a and resizes the padded volume, of extent P_a = n_a + 2 p_a, to `dims`
= m trilinearly with align_corners.  So native index i_a sits at grid coordinate (i_a + p_a) (m_a - 1) / (P_a - 1), and a
normalised displacement of 2 spans m_a - 1 grid voxels = P_a - 1 padded native voxels.  Where max(n) - n_a is odd P_a is
max(n) - 1: the padded volume is not always a cube.  `ops.native_warp` takes a NativeGrid; DESIGN.md section 6 has the
definition of what it computes."""
from collections import namedtuple


class NativeGrid(namedtuple('NativeGrid', 'shape padding padded dims zooms')):
    """shape: the native (n0, n1, n2); padding: voxels added on BOTH sides of each axis; padded: shape + 2 padding; dims: the
    registration grid; zooms: the voxel size in mm per axis of `shape` (the NIfTI header's pixdim[1:4]).  All in the axis order
    of the native array; the per-CHANNEL quantities (`voxel_scale`, `mm_scale`, `spacing_xyz`) run the other way: channel 0
    of a field, and sx of a spacing, belong to the LAST axis."""
    __slots__ = ()

    @classmethod
    def from_shape(cls, native_shape, dims, zooms=(1.0, 1.0, 1.0)):
        shape, dims, zooms = tuple(int(n) for n in native_shape), tuple(int(m) for m in dims), tuple(float(z) for z in zooms)
        if len(shape) != 3 or len(dims) != 3 or len(zooms) != 3:
            raise ValueError(f'native shape, dims and zooms must have three entries each, got {shape}, {dims}, {zooms}')
        if min(shape) < 1 or min(dims) < 2:
            raise ValueError(f'native shape {shape} needs every axis >= 1 and dims {dims} every axis >= 2')
        if not all(z > 0 and z != float('inf') for z in zooms):
            raise ValueError(f'zooms must be finite and > 0, got {zooms}')
        padding = tuple((max(shape) - n) // 2 for n in shape)   # what BiobankDataset._padded pads with, per side
        padded = tuple(n + 2 * p for n, p in zip(shape, padding))
        if min(padded) < 2:
            raise ValueError(f'native shape {shape}: the padded extent {padded} needs every axis >= 2')
        return cls(shape, padding, padded, dims, zooms)

    def grid_coordinate(self, i):
        """the registration-grid coordinate (in grid voxels, per axis) of the native index i = (i0, i1, i2)"""
        return tuple((ia + p) * (m - 1) / (P - 1) for ia, p, m, P in zip(i, self.padding, self.dims, self.padded))

    def voxel_scale(self):
        """normalised displacement -> native voxels, per CHANNEL: (P2 - 1) / 2, (P1 - 1) / 2, (P0 - 1) / 2"""
        return tuple((P - 1) / 2 for P in reversed(self.padded))

    def mm_scale(self):
        """normalised displacement -> mm, per CHANNEL: the voxel scale times the zoom of the channel's axis"""
        return tuple(s * z for s, z in zip(self.voxel_scale(), reversed(self.zooms)))

    def spacing_xyz(self):
        """the zooms as (sx, sy, sz) of ops.label_surface_distance / label_hausdorff_distance, where sx scales the LAST axis:
        (zooms[2], zooms[1], zooms[0])"""
        return tuple(reversed(self.zooms))
