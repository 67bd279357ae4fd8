"""The numpy restatement of the mask operators (tests/_masks.py) against scipy.ndimage, with exact equality; the host-side parts of
ir_sgmcmc_amd/masks.py (Otsu threshold, option parser) and the `optional` directories of BiobankDataset.  No GPU."""
import itertools
import logging

import numpy as np
import pytest
import torch
from scipy import ndimage

from ir_sgmcmc_amd import masks as M
from ir_sgmcmc_amd.data_loader.data_loaders import BiobankDataLoader
from ir_sgmcmc_amd.data_loader.datasets import BiobankDataset
from ir_sgmcmc_amd.utils.imageio import write_nifti
from tests import _masks as S

SHAPES = [(19, 21, 70), (2, 9, 67), (33, 5, 5)]
STRUCTURES = {6: 1, 18: 2, 26: 3}  # ndimage.generate_binary_structure(3, k)


def bernoulli(shape, p, seed):
    return np.random.default_rng(seed).random(shape) < p


def blobs(shape, seed, n=4):
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*(np.arange(s) for s in shape), indexing='ij')
    out = np.zeros(shape, bool)
    for _ in range(n):
        c = [rng.uniform(0, s - 1) for s in shape]
        r = rng.uniform(1.5, max(2.0, min(shape) / 2))
        out |= (z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2 <= r * r
    return out


# ---- the restatement against scipy
@pytest.mark.parametrize('connectivity', [6, 18, 26])
@pytest.mark.parametrize('shape', SHAPES[1:] + [(9, 10, 11)])
@pytest.mark.parametrize('p', [0.2, 0.5, 0.8])
def test_components_equal_scipy_label(shape, p, connectivity):
    mask = bernoulli(shape, p, seed=3)
    labels, n = S.connected_components(mask, connectivity)
    ref, n_ref = ndimage.label(mask, ndimage.generate_binary_structure(3, STRUCTURES[connectivity]))
    assert n == n_ref
    assert np.array_equal(labels, S.canonical_labels(ref))  # scipy's labels canonicalised: its numbering is not relied upon


def test_canonical_labels_renumbers_by_first_occurrence():
    labels = np.array([[[0, 7, 7], [2, 0, 7]], [[2, 0, 5], [0, 5, 5]]])
    assert np.array_equal(S.canonical_labels(labels), np.array([[[0, 1, 1], [2, 0, 1]], [[2, 0, 3], [0, 3, 3]]]))


@pytest.mark.parametrize('shape', SHAPES[1:] + [(9, 10, 11)])
def test_fill_holes_equals_scipy(shape):
    for seed, p in itertools.product(range(2), (0.5, 0.8)):
        mask = bernoulli(shape, p, seed)
        assert np.array_equal(S.fill_holes(mask), ndimage.binary_fill_holes(mask))
    shell = np.zeros((9, 10, 11), bool)
    shell[2:7, 2:8, 2:9] = True
    shell[3:6, 3:7, 3:8] = False
    assert np.array_equal(S.fill_holes(shell), ndimage.binary_fill_holes(shell)) and S.fill_holes(shell)[4, 5, 5]


@pytest.mark.parametrize('radius', [1, 1.5, 2, 3.7, 8, 16])
@pytest.mark.parametrize('shape', [(2, 9, 67), (33, 5, 5), (12, 13, 20)])
def test_dilation_equals_the_distance_transform(shape, radius):
    r2 = S.ball_r2(radius)
    for mask in (bernoulli(shape, 0.01, 5), blobs(shape, 6)):
        if not mask.any():
            mask[tuple(s // 2 for s in shape)] = True
        edt = ndimage.distance_transform_edt(~mask)  # the distance of every voxel to the nearest set voxel
        assert np.array_equal(S.dilate(mask, radius), np.rint(edt ** 2) <= r2)
        assert np.array_equal(S.erode(mask, radius), ~S.dilate(~mask, radius))


def test_ball_r2_rounds_down_after_a_guard():
    assert [S.ball_r2(r) for r in (0, 1, 1.5, 2, 3.7, 8, 16, np.sqrt(2), np.sqrt(3))] == [0, 1, 2, 4, 13, 64, 256, 2, 3]
    assert [M.ball_r2(r) for r in (0, 1, 1.5, 2, 3.7, 8, 16, float(np.sqrt(2)), float(np.sqrt(3)))] == [0, 1, 2, 4, 13, 64, 256, 2, 3]
    with pytest.raises(RuntimeError, match='up to 16'):
        M.ball_r2(17)
    with pytest.raises(RuntimeError, match='radius'):
        M.ball_r2(-1)


def test_erosion_does_not_eat_from_the_border():
    full = np.ones((5, 6, 7), bool)
    assert S.erode(full, 2).all()
    full[2, 3, 3] = False
    assert int((~S.erode(full, 1)).sum()) == 7


def test_keep_largest_ties_go_to_the_first_component():
    mask = np.zeros((3, 3, 12), bool)
    mask[0, 0, 0:3] = mask[1, 1, 4:7] = True
    mask[2, 2, 9:11] = True
    assert np.array_equal(np.argwhere(S.keep_largest(mask, 6, 1))[:, 2], [0, 1, 2])
    assert int(S.keep_largest(mask, 6, 2).sum()) == 6 and np.array_equal(S.keep_largest(mask, 6, 5), mask)


def test_histogram_restatement_counts_every_finite_voxel():
    rng = np.random.default_rng(0)
    im = rng.normal(size=(5, 6, 7)).astype(np.float32)
    im[0, 0, 0] = np.nan
    h = S.intensity_histogram(im, 16, (float(np.nanmin(im)), float(np.nanmax(im))))
    assert h.sum() == im.size - 1 and h[0] >= 1 and h[-1] >= 1
    ref, _ = np.histogram(im[np.isfinite(im)], 16, (float(np.nanmin(im)), float(np.nanmax(im))))
    assert np.abs(h - ref).sum() <= 4  # the fp32 rule and numpy's float64 edges differ at most where a value sits on an edge


# ---- Otsu
def test_otsu_bimodal_histogram_has_the_known_edge():
    counts = np.array([0, 40, 60, 0, 0, 0, 0, 50, 30, 0])
    # every edge between the two modes separates the same classes: the lowest of them, edge 3 of [0, 10) -> 3.0
    assert M.otsu_threshold(counts, (0.0, 10.0)) == 3.0 == S.otsu_threshold(counts, (0.0, 10.0))
    skew = np.array([100, 5, 1, 0, 1, 7, 90, 3])
    assert M.otsu_threshold(skew, (-4.0, 4.0)) == S.otsu_threshold(skew, (-4.0, 4.0))
    assert M.otsu_threshold(torch.tensor(skew).reshape(1, -1), (-4.0, 4.0)) == S.otsu_threshold(skew, (-4.0, 4.0))


def test_otsu_tie_goes_to_the_lowest_edge():
    assert M.otsu_threshold([5, 0, 0, 5], (0.0, 4.0)) == 1.0
    assert M.otsu_threshold([3, 3], (2.0, 4.0)) == 3.0


def test_otsu_random_histograms_match_the_loop():
    rng = np.random.default_rng(1)
    for bins in (2, 3, 17, 64):
        counts = rng.integers(0, 50, bins)
        counts[:2] += 1
        assert M.otsu_threshold(counts, (-1.0, 2.5)) == pytest.approx(S.otsu_threshold(counts, (-1.0, 2.5)), abs=1e-12)


def test_otsu_refusals():
    with pytest.raises(ValueError, match='empty'):
        M.otsu_threshold([0, 0, 0], (0.0, 1.0))
    with pytest.raises(ValueError, match='single occupied bin'):
        M.otsu_threshold([0, 9, 0], (0.0, 1.0))
    with pytest.raises(ValueError, match='at least 2 bins'):
        M.otsu_threshold([4], (0.0, 1.0))
    with pytest.raises(ValueError, match='one histogram'):
        M.otsu_threshold(np.ones((2, 4)), (0.0, 1.0))
    with pytest.raises(ValueError, match='hi > lo'):
        M.otsu_threshold([1, 2], (1.0, 1.0))
    with pytest.raises(ValueError, match='negative'):
        M.otsu_threshold([1, -2], (0.0, 1.0))


# ---- the option parser
def test_auto_mask_absent_is_none_and_defaults_fill_in():
    assert M.auto_mask_options({}) is None and M.auto_mask_options({'auto_mask': None}) is None
    assert M.auto_mask_options({'auto_mask': {}}) == M.AUTO_MASK_DEFAULTS
    opt = M.auto_mask_options({'auto_mask': {'source': 'file', 'which': 'fixed', 'threshold': 3, 'bins': 64, 'connectivity': 6,
                                             'keep': 2, 'fill_holes': False, 'closing': 0, 'dilation': 2.5, 'save': False}})
    assert opt == {'source': 'file', 'which': 'fixed', 'threshold': 3.0, 'bins': 64, 'connectivity': 6, 'keep': 2,
                   'fill_holes': False, 'closing': 0.0, 'dilation': 2.5, 'save': False}
    assert M.auto_mask_sides(opt) == ('fixed',) and M.auto_mask_sides(M.AUTO_MASK_DEFAULTS) == ('fixed', 'moving')


@pytest.mark.parametrize('key, bad', [
    ('source', 'images'), ('source', 1), ('which', 'all'), ('threshold', 'li'), ('threshold', True), ('threshold', float('nan')),
    ('bins', 1), ('bins', 4097), ('bins', 64.0), ('bins', True), ('connectivity', 8), ('connectivity', True), ('keep', 0),
    ('keep', 65), ('keep', 1.5), ('fill_holes', 1), ('save', 'yes'), ('closing', -1), ('closing', 17), ('closing', '2'),
    ('dilation', 16.5), ('dilation', True), ('dilation', float('inf'))])
def test_auto_mask_refusals_name_the_key(key, bad):
    with pytest.raises(ValueError, match=rf'trainer\.auto_mask\.{key}\b'):
        M.auto_mask_options({'auto_mask': {key: bad}})


def test_auto_mask_refuses_unknown_keys_and_other_types():
    with pytest.raises(ValueError, match=r"unknown keys \['erosion'\]"):
        M.auto_mask_options({'auto_mask': {'erosion': 1}})
    with pytest.raises(ValueError, match='must be an object'):
        M.auto_mask_options({'auto_mask': True})


def test_operators_refuse_cpu_tensors_and_wrong_shapes():
    mask = torch.ones(1, 1, 4, 4, 4, dtype=torch.bool)
    for call in (lambda: M.connected_components(mask), lambda: M.keep_largest(mask), lambda: M.fill_holes(mask),
                 lambda: M.dilate(mask, 1), lambda: M.intensity_histogram(mask.float(), value_range=(0, 1)),
                 lambda: M.threshold_mask(mask.float(), 0.5)):
        with pytest.raises(RuntimeError, match='GPU only'):
            call()
    with pytest.raises(RuntimeError, match=r'\(C,1,D,H,W\)'):
        M.connected_components(mask[0])
    with pytest.raises(RuntimeError, match='bool or uint8'):
        M.fill_holes(mask.float())
    with pytest.raises(RuntimeError, match='6, 18 or 26'):
        M.connected_components(mask, 8)
    with pytest.raises(RuntimeError, match='keep'):
        M.keep_largest(mask, 26, 0)


# ---- the optional directories of the data set
def biobank_dir(root, masks=True, segs=True, empty=()):
    rng = np.random.default_rng(0)
    for name in ('a', 'b'):
        write_nifti(rng.random((6, 7, 8)).astype(np.float32), str(root / f'{name}.nii.gz'))
    for sub, on in (('masks', masks), ('segs', segs)):
        if on or sub in empty:
            (root / sub).mkdir()
        if on:
            for name in ('a', 'b'):
                write_nifti((rng.random((6, 7, 8)) > 0.5).astype(np.uint8), str(root / sub / f'{name}.nii.gz'))
    return str(root)


def test_dataset_without_optional_keeps_its_error(tmp_path):
    d = biobank_dir(tmp_path, masks=False, segs=False)
    with pytest.raises(FileNotFoundError, match='need at least two image / mask / seg triples'):
        BiobankDataset((8, 8, 8), d)
    with pytest.raises(FileNotFoundError, match='need at least two image / mask / seg triples'):
        BiobankDataset((8, 8, 8), d, optional=('segs',))
    with pytest.raises(FileNotFoundError, match='no usable image pair'):
        BiobankDataLoader(d, (8, 8, 8))
    with pytest.raises(ValueError, match='optional'):
        BiobankDataset((8, 8, 8), d, optional=('images',))


def test_dataset_optional_masks_and_segs(tmp_path, caplog):
    d = biobank_dir(tmp_path, masks=False, segs=False, empty=('segs',))
    with caplog.at_level(logging.WARNING, logger='default'):
        dl = BiobankDataLoader(d, (8, 8, 8), optional=['masks', 'segs'])
    assert (dl.has_masks, dl.has_segs) == (False, False)
    assert sum('no files under' in r.getMessage() for r in caplog.records) == 2
    fixed, moving, vp = next(iter(dl))
    for side in (fixed, moving):
        assert sorted(side) == ['im', 'mask'] and side['mask'].dtype == torch.bool and bool(side['mask'].all())
        assert side['mask'].shape == side['im'].shape == (1, 1, 8, 8, 8)
    with pytest.raises(FileNotFoundError, match='native-resolution pair needs'):
        dl.native()


def test_dataset_optional_reads_what_is_there(tmp_path):
    d = biobank_dir(tmp_path, masks=True, segs=False)
    dl = BiobankDataLoader(d, (8, 8, 8), optional=['masks', 'segs'])
    assert (dl.has_masks, dl.has_segs) == (True, False)
    fixed, moving, _ = next(iter(dl))
    assert sorted(fixed) == ['im', 'mask'] and not bool(fixed['mask'].all())
    (tmp_path / 'full').mkdir()
    full = BiobankDataLoader(biobank_dir(tmp_path / 'full'), (8, 8, 8), optional=['masks', 'segs'])
    fixed, _, _ = next(iter(full))
    assert sorted(fixed) == ['im', 'mask', 'seg'] and (full.has_masks, full.has_segs) == (True, True)
