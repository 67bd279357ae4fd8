"""The mask operators of ir_sgmcmc_amd/masks.py on the GPU against the numpy restatement of tests/_masks.py (which shares no code
with the HIP path and is itself held against scipy.ndimage in tests/test_masks_host.py).  Every comparison is exact: labels,
counts and masks are integers.  Shapes: no extent a multiple of the 32 x 8 x 4 tile of the labelling or of the 64 x 4 block of
the pointwise kernels, one extent above 64 (two wavefronts, three tiles along x), one extent of 2; more than one 1024-voxel block
of the root scan; C = 1 and C = 3 volumes of different content."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from ir_sgmcmc_amd import _lib as L
from ir_sgmcmc_amd import masks as M
from ir_sgmcmc_amd.data_loader import synthetic_pair
from tests import _masks as S

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SHAPES = [(19, 21, 70), (2, 9, 67), (33, 5, 5)]
CONNECTIVITIES = (6, 18, 26)


def dev(volumes):
    """(C,D,H,W) bool array -> (C,1,D,H,W) bool tensor on the device"""
    return torch.from_numpy(np.ascontiguousarray(volumes)).unsqueeze(1).to(DEV)


def host(t):
    return t[:, 0].cpu().numpy()


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


def check_components(volumes, connectivity):
    """the labels and counts of a (C,D,H,W) batch against the flood fill, volume by volume -> the counts"""
    labels, counts = M.connected_components(dev(volumes), connectivity)
    assert labels.dtype == torch.int32 and counts.dtype == torch.int32 and labels.shape == (len(volumes), 1, *volumes.shape[1:])
    labels, counts = host(labels), counts.cpu().numpy()
    for c, volume in enumerate(volumes):
        ref, n = S.connected_components(volume, connectivity)
        assert counts[c] == n and np.array_equal(labels[c], ref), (c, connectivity, counts[c], n)
    return counts


# ---- components
@pytest.mark.parametrize('p', [0.2, 0.5, 0.8])
@pytest.mark.parametrize('shape', SHAPES)
def test_components_of_bernoulli_masks(shape, p):
    volumes = np.stack([bernoulli(shape, p, seed) for seed in range(3)])  # three seeds: one batch of C = 3
    for connectivity in CONNECTIVITIES:
        check_components(volumes, connectivity)
    check_components(volumes[1:2], 26)  # C = 1


def test_face_edge_and_corner_neighbours_separate_the_connectivities():
    shape, a = SHAPES[0], (3, 7, 31)  # the second voxel lies across a tile face in z, y and x
    volumes = np.zeros((3, *shape), bool)
    for c, off in enumerate(((0, 0, 1), (0, 1, 1), (1, 1, 1))):
        volumes[c][a] = volumes[c][tuple(i + o for i, o in zip(a, off))] = True
    assert [list(check_components(volumes, k)) for k in CONNECTIVITIES] == [[1, 2, 2], [1, 1, 2], [1, 1, 1]]
    inside = np.zeros((3, 6, 6, 6), bool)  # the same inside one tile
    for c, off in enumerate(((0, 0, 1), (0, 1, 1), (1, 1, 1))):
        inside[c][1, 1, 1] = inside[c][tuple(1 + o for o in off)] = True
    assert [list(check_components(inside, k)) for k in CONNECTIVITIES] == [[1, 2, 2], [1, 1, 2], [1, 1, 1]]


@pytest.mark.parametrize('shape', SHAPES)
def test_nothing_connects_across_a_row_a_plane_or_a_volume(shape):
    D, H, W = shape
    volumes = np.zeros((3, *shape), bool)
    volumes[0][0, 0, W - 1] = volumes[0][0, 1, 0] = True          # the end of a row and the start of the next
    volumes[1][0, H - 1, W - 1] = volumes[1][1, 0, 0] = True      # the end of a plane and the start of the next
    volumes[1][D - 1, H - 1, W - 1] = volumes[2][0, 0, 0] = True  # the end of a volume and the start of the next
    for connectivity in CONNECTIVITIES:
        # (with D = 2 the last voxels of the two planes are neighbours by a face)
        assert list(check_components(volumes, connectivity)) == [2, 3 if D > 2 else 2, 1]


def serpentine(shape):
    """a one-voxel-wide path through the whole volume: every other row of every other plane, joined at alternating ends"""
    D, H, W = shape
    m = np.zeros(shape, bool)
    for z in range(0, D, 2):
        for y in range(0, H, 2):
            m[z, y, :] = True
            if y + 2 < H:
                m[z, y + 1, W - 1 if (y // 2) % 2 == 0 else 0] = True
        if z + 2 < D:
            last_y = (H - 1) // 2 * 2
            m[z + 1, last_y if (z // 2) % 2 == 0 else 0, W - 1 if ((H - 1) // 2) % 2 == 0 else 0] = True
    return m


def test_long_merge_chains():
    snake = serpentine((17, 17, 33))
    comb = np.zeros((17, 17, 33), bool)
    comb[:, ::2, ::2] = True  # teeth along z ...
    open_comb = comb.copy()
    comb[16] = True           # ... that join only in the last plane
    z, y, x = np.meshgrid(np.arange(17), np.arange(17), np.arange(33), indexing='ij')
    lattice = ((y % 3 == 0) & (x % 3 == 0)) | ((z % 3 == 0) & (x % 3 == 0)) | ((z % 3 == 0) & (y % 3 == 0))  # crosses every tile face
    volumes = np.stack([snake, comb, open_comb, lattice])
    assert list(check_components(volumes, 6)) == [1, 1, 9 * 17, 1]
    check_components(volumes, 26)
    # the longest chain there is: one row of 70 across three tiles, and the snake through the big shape
    check_components(np.stack([serpentine(SHAPES[0])]), 6)


@pytest.mark.parametrize('shape', SHAPES)
def test_empty_full_and_single_voxel_masks(shape):
    volumes = np.zeros((3, *shape), bool)
    volumes[1] = True
    volumes[2][tuple(s - 1 for s in shape)] = True
    for connectivity in CONNECTIVITIES:
        assert list(check_components(volumes, connectivity)) == [0, 1, 1]
    for op in (M.keep_largest, M.fill_holes):
        assert np.array_equal(host(op(dev(volumes))), volumes)


def test_two_calls_are_bit_identical_and_uint8_comes_back_uint8():
    m = dev(np.stack([bernoulli(SHAPES[0], 0.5, 7)]))
    a, b = M.connected_components(m, 18), M.connected_components(m, 18)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    u8 = m.to(torch.uint8) * 255
    assert torch.equal(M.connected_components(u8, 18)[0], a[0])
    for op in (M.keep_largest, M.fill_holes, lambda t: M.dilate(t, 1.5), lambda t: M.erode(t, 1)):
        out = op(u8)
        assert out.dtype == torch.uint8 and int(out.max()) <= 1 and torch.equal(out.bool(), op(m))


# ---- keep_largest
@pytest.mark.parametrize('shape', SHAPES)
def test_keep_largest(shape):
    volumes = np.stack([bernoulli(shape, 0.2, 11), blobs(shape, 12), bernoulli(shape, 0.5, 13)])
    for connectivity, keep in ((6, 1), (6, 2), (26, 1), (18, 3), (26, 64)):
        out = host(M.keep_largest(dev(volumes), connectivity, keep))
        for c, volume in enumerate(volumes):
            assert np.array_equal(out[c], S.keep_largest(volume, connectivity, keep)), (c, connectivity, keep)


def test_keep_largest_tie_and_more_than_there_are():
    m = np.zeros((1, 5, 9, 70), bool)
    m[0, 4, 8, 60:63] = True   # three components of 3, 3 and 2 voxels: the tie goes to the one that starts first
    m[0, 0, 0, 3:6] = True
    m[0, 2, 4, 33:35] = True
    one = host(M.keep_largest(dev(m), 6, 1))
    assert int(one.sum()) == 3 and one[0, 0, 0, 3:6].all()
    two = host(M.keep_largest(dev(m), 6, 2))
    assert int(two.sum()) == 6 and not two[0, 2, 4, 33:35].any()
    assert np.array_equal(host(M.keep_largest(dev(m), 6, 3)), m) and np.array_equal(host(M.keep_largest(dev(m), 6, 50)), m)
    with pytest.raises(L.IrsError, match='keep'):
        M.keep_largest(dev(m), 6, 65)


# ---- fill_holes
def shell(shape=(12, 13, 40)):
    m = np.zeros(shape, bool)
    m[2:10, 2:11, 2:38] = True
    m[3:9, 3:10, 3:37] = False
    return m


def test_fill_holes_shells():
    closed = shell()
    leak = shell()
    leak[2, 6, 20] = False       # a one-voxel 6-connected leak: nothing is filled
    diagonal = shell()
    diagonal[2, 2, 2] = False    # the corner voxel: the cavity reaches the outside only diagonally -> still filled
    cavity = np.zeros((12, 13, 40), bool)
    cavity[0:6, 3:9, 5:30] = True
    cavity[0:5, 4:8, 6:29] = False  # a cavity that touches the border plane z = 0
    volumes = np.stack([closed, leak, diagonal, cavity])
    out = host(M.fill_holes(dev(volumes)))
    for c, volume in enumerate(volumes):
        assert np.array_equal(out[c], S.fill_holes(volume)), c
    assert out[0][3:9, 3:10, 3:37].all() and np.array_equal(out[1], leak) and out[2][3:9, 3:10, 3:37].all()
    assert not out[2][2, 2, 2] and np.array_equal(out[3], cavity)


@pytest.mark.parametrize('shape', SHAPES)
def test_fill_holes_of_random_masks(shape):
    volumes = np.stack([bernoulli(shape, 0.5, 21), bernoulli(shape, 0.8, 22), blobs(shape, 23) & ~blobs(shape, 24, 2)])
    out = host(M.fill_holes(dev(volumes)))
    for c, volume in enumerate(volumes):
        assert np.array_equal(out[c], S.fill_holes(volume)), c


# ---- morphology
@functools.lru_cache(maxsize=None)
def morphology_volumes(shape):
    touching = np.zeros(shape, bool)  # a mask that touches every face of the volume
    touching[0], touching[-1], touching[:, 0], touching[:, -1], touching[:, :, 0], touching[:, :, -1] = (True,) * 6
    touching[tuple(s // 2 for s in shape)] = True
    sparse = bernoulli(shape, 0.01, 31)
    sparse[tuple(s // 3 for s in shape)] = True
    return np.stack([sparse, blobs(shape, 32), touching])


@pytest.mark.parametrize('radius', [0, 1, 1.5, 2, 3.7, 8, 16])
@pytest.mark.parametrize('shape', SHAPES)
def test_dilate_and_erode(shape, radius):
    volumes = morphology_volumes(shape)
    m = dev(volumes)
    grown, shrunk = M.dilate(m, radius), M.erode(m, radius)
    for c, volume in enumerate(volumes):
        assert np.array_equal(host(grown)[c], S.dilate(volume, radius)), (c, 'dilate')
        assert np.array_equal(host(shrunk)[c], S.erode(volume, radius)), (c, 'erode')
    assert torch.equal(shrunk, ~M.dilate(~m, radius))
    if radius == 0:
        assert torch.equal(grown, m) and torch.equal(M.dilate(grown, 0), grown)
    assert torch.equal(M.dilate(m[1:2], radius), grown[1:2])  # C = 1


@pytest.mark.parametrize('radius', [1, 2, 3.7])
@pytest.mark.parametrize('shape', SHAPES)
def test_close_and_open(shape, radius):
    volumes = morphology_volumes(shape)
    m = dev(volumes)
    closed, opened = M.close(m, radius), M.open(m, radius)
    for c, volume in enumerate(volumes):
        assert np.array_equal(host(closed)[c], S.close(volume, radius)) and np.array_equal(host(opened)[c], S.open(volume, radius))
    assert bool((closed | ~m).all()) and bool((m | ~opened).all())  # close >= m >= open
    assert torch.equal(M.close(m, radius), closed)


def test_radius_17_is_refused():
    m = dev(np.ones((1, 4, 5, 6), bool))
    for op in (M.dilate, M.erode, M.close, M.open):
        with pytest.raises(L.IrsError, match='up to 16'):
            op(m, 17)
    u8, out, ws = m.view(torch.uint8), torch.empty(120, dtype=torch.uint8, device=DEV), torch.empty(4096, dtype=torch.uint8, device=DEV)
    lib = L.load()
    assert lib.irs_mask_dilate(L.dev_ptr(u8), 1, 4, 5, 6, 289, 0, L.dev_ptr(out), L.dev_ptr(ws), 4096, L.stream_ptr()) != 0
    assert b'at most 16' in lib.irs_last_error()


def test_abi_refusals():
    lib, st = L.load(), L.stream_ptr()
    m = dev(np.ones((1, 4, 5, 6), bool)).view(torch.uint8)
    labels = torch.empty(120, dtype=torch.int32, device=DEV)
    counts = torch.empty(1, dtype=torch.int32, device=DEV)
    nbytes = C.c_size_t()
    assert lib.irs_connected_components_workspace(1, 4, 5, 6, C.byref(nbytes)) == 0 and nbytes.value >= 2 * 120 * 4
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=DEV)
    call = lambda *a: lib.irs_connected_components(*a, st)
    assert call(L.dev_ptr(m), 1, 4, 5, 6, 26, L.dev_ptr(labels), L.dev_ptr(counts), L.dev_ptr(ws), nbytes.value) == 0
    for args, text in (((L.dev_ptr(m), 1, 4, 5, 6, 8, L.dev_ptr(labels), L.dev_ptr(counts), L.dev_ptr(ws), nbytes.value), b'6, 18 or 26'),
                       ((L.dev_ptr(m), 1, 4, 5, 6, 26, L.dev_ptr(labels), L.dev_ptr(counts), L.dev_ptr(ws), nbytes.value - 1), b'workspace'),
                       ((L.dev_ptr(m), 0, 4, 5, 6, 26, L.dev_ptr(labels), L.dev_ptr(counts), L.dev_ptr(ws), nbytes.value), b'volumes'),
                       ((L.dev_ptr(m), 1, 0, 5, 6, 26, L.dev_ptr(labels), L.dev_ptr(counts), L.dev_ptr(ws), nbytes.value), b'>= 1'),
                       ((None, 1, 4, 5, 6, 26, L.dev_ptr(labels), L.dev_ptr(counts), L.dev_ptr(ws), nbytes.value), b'null'),
                       ((L.dev_ptr(m), 1, 1 << 10, 1 << 10, 1 << 10, 26, L.dev_ptr(labels), L.dev_ptr(counts), L.dev_ptr(ws), nbytes.value),
                        b'2^30')):
        assert call(*args) != 0 and text in lib.irs_last_error(), text
    assert lib.irs_connected_components_workspace(1, 1 << 10, 1 << 10, 1 << 10, C.byref(nbytes)) != 0


# ---- histogram and threshold
@pytest.mark.parametrize('shape', SHAPES)
def test_intensity_histogram_is_exact(shape):
    rng = np.random.default_rng(41)
    ims = rng.normal(size=(3, *shape)).astype(np.float32)
    ims[1] = np.round(ims[1] * 4) / 4      # many voxels on bin edges and in one bin
    ims[2, 0, 0, :5] = [np.nan, np.inf, -np.inf, 9.0, -9.0]
    mask = bernoulli((3, *shape), 0.6, 42)
    t = torch.from_numpy(ims).unsqueeze(1).to(DEV)
    for bins, value_range in ((256, (-3.0, 3.0)), (7, (-0.5, 2.25)), (4096, (-4.0, 4.0))):
        for use, mk in ((None, None), (mask, dev(mask)), (mask[:1], dev(mask[:1]))):
            h = M.intensity_histogram(t, bins, value_range, mk).cpu().numpy()
            assert h.dtype == np.int64
            for c in range(3):
                ref = S.intensity_histogram(ims[c], bins, value_range, None if use is None else use[c if len(use) == 3 else 0])
                assert np.array_equal(h[c], ref), (bins, c)
    lo, hi = float(ims[0].min()), float(ims[0].max())
    assert np.array_equal(M.intensity_histogram(t[:1], 64).cpu().numpy()[0], S.intensity_histogram(ims[0], 64, (lo, hi)))
    assert np.array_equal(host(M.threshold_mask(t, 0.25)), ims > np.float32(0.25))


# ---- the pipeline
def speckled_image(N):
    fixed, _ = synthetic_pair((N, N, N), seed=0)
    im = fixed['im'][0].numpy().copy()
    c = N // 2
    im[c - 1:c + 2, c - 1:c + 2, c - 1:c + 2] = 0.0          # a punched hole in the middle of the blob
    specks = [(1, 1, 1), (2, N - 3, 3), (N - 2, 2, N - 4), (N - 3, N - 3, N - 3)]
    for s in specks:
        im[s] = 2.0                                           # bright specks far from it
    return im, specks


@pytest.mark.parametrize('N', [32, 48])
def test_foreground_mask_of_the_synthetic_image(N):
    im, specks = speckled_image(N)
    t = torch.from_numpy(im).reshape(1, 1, N, N, N).to(DEV)
    mask, summary = M.foreground_mask(t, closing=2, dilation=1)
    value_range = (float(im.min()), float(im.max()))
    assert summary['threshold'] == S.otsu_threshold(S.intensity_histogram(im, 256, value_range), value_range)
    ref, voxels = S.foreground_mask(im, summary['threshold'], 26, 1, True, 2, 1)
    assert np.array_equal(host(mask)[0], ref) and summary['voxels'] == voxels and list(summary['voxels']) == list(voxels)
    assert summary['components'] == S.connected_components(im > np.float32(summary['threshold']), 26)[1] >= 1 + len(specks)
    assert summary['total'] == N ** 3
    nz = np.nonzero(ref)
    assert summary['bounding_box'] == [[int(a.min()), int(a.max()) + 1] for a in nz]
    got = host(mask)[0]
    assert not any(got[s] for s in specks) and got[N // 2, N // 2, N // 2]  # the specks are gone, the hole is filled
    assert not (im > np.float32(summary['threshold']))[N // 2, N // 2, N // 2]
    again, summary2 = M.foreground_mask(t, closing=2, dilation=1)
    assert torch.equal(again, mask) and summary2 == summary
    fixed_mask, s3 = M.foreground_mask(t, threshold=0.5, fill_holes=False, closing=0, dilation=0, keep=2, connectivity=6)
    ref3, voxels3 = S.foreground_mask(im, 0.5, 6, 2, False, 0, 0)
    assert np.array_equal(host(fixed_mask)[0], ref3) and s3['voxels'] == voxels3 and s3['threshold'] == 0.5


def test_foreground_mask_names_the_stage_that_fails():
    t = torch.zeros(1, 1, 8, 9, 10, device=DEV)
    t[0, 0, 2:5, 2:5, 2:5] = 1.0
    with pytest.raises(ValueError, match='is empty after the stage "threshold"'):
        M.foreground_mask(t, threshold=2.0)
    with pytest.raises(ValueError, match='covers the whole volume after the stage "threshold"'):
        M.foreground_mask(t, threshold=-1.0)
    with pytest.raises(ValueError, match='covers the whole volume after the stage "dilation"'):
        M.foreground_mask(t, threshold=0.5, dilation=16)
    with pytest.raises(L.IrsError, match='hi > lo'):  # a constant image has no range to bin
        M.foreground_mask(torch.ones(1, 1, 8, 9, 10, device=DEV))
