"""BiobankDataset (reference data_loader/datasets.py:13-145) on top of the numpy NIfTI reader.

Directory layout as in the reference: `<data_dir>/*.nii.gz` images, `<data_dir>/masks/*`, `<data_dir>/segs/*`, sorted by
name; image 0 is the fixed image, image idx + 1 the moving one (all-to-one, `__len__` = 1).  Every volume is padded with
its minimum to a cube of the largest extent, then resized to `dims`: trilinear / align_corners for images, nearest for
masks and segmentations -- the same torch calls the reference makes (:70-105)."""
import json
import logging
import os
from os import listdir, path

import numpy as np
import torch
import torch.nn.functional as F

from ..native import NativeGrid
from ..ops import control_grid_size
from ..utils.imageio import read_nifti


class BiobankDataset:
    OPTIONAL = ('masks', 'segs')  # the directories `optional` may list

    def __init__(self, dims, im_paths, save_paths=None, sigma_v_init=0.5, u_v_init=0.1, cps=None, optional=()):
        """optional: the directories out of OPTIONAL that may be missing or empty (absent in the reference, which needs both).
        Without masks every mask is all-true; without segs the pair has no 'seg' key.  One warning each.  `native_pair` keeps
        requiring its files."""
        if isinstance(optional, str) or any(name not in self.OPTIONAL for name in optional):
            raise ValueError(f'optional must be a list out of {list(self.OPTIONAL)}, got {optional!r}')
        self.im_paths, self.save_paths = im_paths, save_paths
        self.sigma_v_init, self.u_v_init = sigma_v_init, u_v_init
        self.dims = tuple(dims)
        self.dims_im = (1, *self.dims)
        self.dims_v = (3, *self.dims) if cps is None else (3, *control_grid_size(self.dims, cps))
        self.padding, self.im_spacing = None, None
        self.zooms = None  # the header zooms of the first volume read, in the axis order of its array

        im_filenames = self._get_filenames(im_paths)
        mask_filenames = self._get_filenames(path.join(im_paths, 'masks'))
        seg_filenames = self._get_filenames(path.join(im_paths, 'segs'))
        # an optional directory that is missing or empty is left out of the triples (a directory with files in it is read and
        # checked as ever)
        self.has_masks = not ('masks' in optional and not any(mask_filenames))
        self.has_segs = not ('segs' in optional and not any(seg_filenames))
        for present, name, instead in ((self.has_masks, 'masks', 'every mask is all-true'), (self.has_segs, 'segs', "the pair has no 'seg'")):
            if not present:
                logging.getLogger('default').warning(f'BiobankDataset: no files under {path.join(im_paths, name)}: {instead}')
        columns = {'im': im_filenames}
        if self.has_masks:
            columns['mask'] = mask_filenames
        if self.has_segs:
            columns['seg'] = seg_filenames
        self.im_mask_seg_triples = [dict(zip(columns, t)) for t in zip(*columns.values())]
        if len(self.im_mask_seg_triples) < 2 or any(not path.isfile(f) for t in self.im_mask_seg_triples[:2] for f in t.values()):
            raise FileNotFoundError(f'{im_paths}: need at least two image / mask / seg triples (fixed + moving)')
        if save_paths and save_paths.get('dir'):
            with open(os.path.join(str(save_paths['dir']), 'idx_to_biobank_ID.json'), 'w') as out:
                json.dump(dict(enumerate(self.im_mask_seg_triples)), out, indent=4, sort_keys=True)

    def __len__(self):
        return 1

    @staticmethod
    def _get_filenames(p):
        if path.isdir(p) and listdir(p):
            return sorted(path.join(p, f) for f in listdir(p) if path.isfile(path.join(p, f)))
        return ['' for _ in range(2)]

    def _padded(self, file_path):
        arr, zooms = read_nifti(file_path, np.float32)
        if arr.ndim != 3:
            raise ValueError(f'{file_path}: expected a 3-D volume, got shape {arr.shape}')
        if self.zooms is None:
            self.zooms = zooms
        if self.im_spacing is None:
            self.im_spacing = torch.tensor(max(arr.shape) / np.asarray(self.dims), dtype=torch.float32)
        if self.padding is None:
            padding = (max(arr.shape) - np.asarray(arr.shape)) // 2
            self.padding = tuple((int(p), int(p)) for p in padding)
        return torch.from_numpy(np.pad(arr, self.padding, mode='minimum')).unsqueeze(0).unsqueeze(0)

    def _get_image(self, im_path):
        return F.interpolate(self._padded(im_path), size=self.dims, mode='trilinear', align_corners=True).squeeze(0)

    def _get_mask(self, mask_path):
        return F.interpolate(self._padded(mask_path), size=self.dims, mode='nearest').bool().squeeze(0)

    def _get_seg(self, seg_path):
        return F.interpolate(self._padded(seg_path), size=self.dims, mode='nearest').short().squeeze(0)

    def _load(self, triple):
        out = {'im': self._get_image(triple['im'])}
        out['mask'] = self._get_mask(triple['mask']) if 'mask' in triple else torch.ones(out['im'].shape, dtype=torch.bool)
        if 'seg' in triple:
            out['seg'] = self._get_seg(triple['seg'])
        return out

    def native_pair(self, idx=0):
        """The pair at its own resolution (absent in the reference, which keeps the resized volumes only): the files are read
        again here, nothing is held by the data set.  -> {'fixed': {...}, 'moving': {...}, 'grid': NativeGrid, 'fill': {'fixed':
        f, 'moving': f}}; the dicts hold the UNPADDED 'im' float32, 'mask' bool and 'seg' int16 tensors of shape (1, *native
        shape), 'fill' the minimum each image is padded with, and the grid carries the header zooms of the fixed image.  The data
        set applies ONE padding to every volume, so volumes of different shapes are refused."""
        triples = {'fixed': self.im_mask_seg_triples[0], 'moving': self.im_mask_seg_triples[idx + 1]}
        if not (self.has_masks and self.has_segs):
            raise FileNotFoundError(f'{self.im_paths}: the native-resolution pair needs the mask and the segmentation files')
        out, shape, zooms, fill = {}, None, None, {}
        for side, triple in triples.items():
            out[side] = {}
            for key, dtype in (('im', torch.float32), ('mask', torch.bool), ('seg', torch.int16)):
                arr, z = read_nifti(triple[key], np.float32)
                if arr.ndim != 3:
                    raise ValueError(f'{triple[key]}: expected a 3-D volume, got shape {arr.shape}')
                if shape is None:
                    shape, zooms = arr.shape, z
                elif arr.shape != shape:
                    raise ValueError(f'{triple[key]}: shape {arr.shape} differs from {shape} of {triples["fixed"]["im"]}; the '
                                     f'native-resolution outputs need fixed and moving volumes of one shape (the data set pads '
                                     f'them all alike)')
                out[side][key] = torch.from_numpy(arr).to(dtype).unsqueeze(0)
            fill[side] = float(out[side]['im'].min())
        return {**out, 'grid': NativeGrid.from_shape(shape, self.dims, zooms), 'fill': fill}

    def __getitem__(self, idx):
        fixed = self._load(self.im_mask_seg_triples[0])
        moving = self._load(self.im_mask_seg_triples[idx + 1])
        var_v = (self.sigma_v_init ** 2) + torch.zeros(self.dims_v)
        var_params_q_v = {'mu': torch.zeros(self.dims_v), 'log_var': var_v.log(), 'u': self.u_v_init + torch.zeros(self.dims_v)}
        return fixed, moving, var_params_q_v
