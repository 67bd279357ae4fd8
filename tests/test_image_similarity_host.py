"""The intensity-similarity option's host surface: the known answers the device tests rely on, proved from the numpy
restatement alone (tests/_image_similarity.py), the trainer option, the metric names and what the C entry points refuse before
they touch the device.  No GPU needed."""
import copy
import json
import math
import os

import numpy as np
import pytest

from tests import _image_similarity as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_identical_images():
    f, _ = S.random_pair((6, 7, 8), 1, 1, seed=3)
    hist, st = S.reference_one(f[0, 0], f[0, 0], None, 16, (0.0, 1.0), (0.0, 1.0))
    assert st['n'] == f.size and hist.sum() == f.size
    assert np.count_nonzero(hist - np.diag(np.diag(hist))) == 0  # diagonal
    assert st['mse'] == 0.0 and st['nmi'] == 2.0
    assert st['mi'] == st['h_fixed'] == st['h_moving'] == st['h_joint'] > 0.0
    assert st['ncc'] == pytest.approx(1.0, abs=1e-12)


def test_independent_lattice():
    f, m = S.lattice(8, 5)
    assert f.size == 5 * 64
    hist, st = S.reference_one(f, m, None, 8, (0.0, 1.0), (0.0, 1.0))
    assert (hist == 5).all()
    assert st['n_clipped'] == 0 and st['n_nonfinite'] == 0
    assert abs(st['mi']) <= 1e-12
    assert abs(st['h_fixed'] - math.log(8)) <= 1e-12 and abs(st['h_moving'] - math.log(8)) <= 1e-12
    assert abs(st['h_joint'] - math.log(64)) <= 1e-12 and abs(st['nmi'] - 1.0) <= 1e-12


def test_bin_edges():
    b, clipped = S.bin_index(S.EDGE_VALUES, 0.0, 1.0, 8)
    assert b.tolist() == S.EDGE_BINS
    assert clipped.tolist() == [False, False, False, False, False, True, True, False] and clipped.sum() == 2
    assert float(S.EDGE_VALUES[2]) < 0.25  # 0.25 - 2^-26 is a float32 of its own, one ulp under the edge


def test_nonfinite_and_empty():
    f, m = S.random_pair((4, 5, 6), 1, 1, seed=1)
    f[0, 0, 0, 0, 0], m[0, 0, 1, 1, 1], m[0, 0, 0, 0, 0] = np.nan, np.inf, 2.0
    mask = np.ones((4, 5, 6), bool)
    mask[3] = False
    hist, st = S.reference_one(f[0, 0], m[0, 0], mask, 8, (0.0, 1.0), (0.0, 1.0))
    assert st['n_nonfinite'] == 2 and st['n'] == 3 * 5 * 6 - 2 == hist.sum() and st['n_clipped'] == 0  # m = 2 fell with f = NaN
    hist, st = S.reference_one(f[0, 0], m[0, 0], np.zeros((4, 5, 6), bool), 8, (0.0, 1.0), (0.0, 1.0))
    assert st['n'] == 0 and not hist.any() and all(math.isnan(st[k]) for k in S.COLUMNS[3:])
    # constant images: one cell, zero entropy, no variance
    c = np.full((4, 5, 6), 0.5, np.float32)
    hist, st = S.reference_one(c, c * 0.5, None, 8, (0.0, 1.0), (0.0, 1.0))
    assert hist[4, 2] == c.size == hist.sum() and st['h_joint'] == 0.0 and math.isnan(st['nmi']) and math.isnan(st['ncc'])
    assert st['mse'] == 0.0625


# ---------------------------------------------------------------- the option
def test_options_helper_parses():
    from ir_sgmcmc_amd.diagnostics import image_similarity_options as opt
    assert opt({}) is None
    assert opt({'image_similarity': False}) is None and opt({'image_similarity': None}) is None
    assert opt({'image_similarity': True}) == {'bins': 64, 'period': None}
    assert opt({'image_similarity': {}}) == {'bins': 64, 'period': None}
    assert opt({'image_similarity': {'bins': 32}}) == {'bins': 32, 'period': None}
    assert opt({'image_similarity': {'period': 5}}) == {'bins': 64, 'period': 5}
    assert opt({'image_similarity': {'bins': 2, 'period': 1}}) == {'bins': 2, 'period': 1}
    assert opt({'image_similarity': {'bins': 128}})['bins'] == 128


@pytest.mark.parametrize('bad', [1, 'yes', [64], {'bin': 64}, {'bins': 64, 'every': 2}, {'bins': 1}, {'bins': 129}, {'bins': 64.0},
                                 {'bins': True}, {'bins': '64'}, {'period': 0}, {'period': -3}, {'period': 2.5}, {'period': True},
                                 {'period': None}])
def test_options_helper_rejects(bad):
    from ir_sgmcmc_amd.diagnostics import image_similarity_options
    with pytest.raises(ValueError, match='trainer.image_similarity'):
        image_similarity_options({'image_similarity': bad})


def _names(tmp_path, **trainer_over):
    from ir_sgmcmc_amd.parse_config import ConfigParser
    cfg = json.load(open(os.path.join(ROOT, 'configs', 'synthetic_gmm_lognormal.json')))
    cfg['trainer'].update(save_dir=str(tmp_path), **trainer_over)
    config = ConfigParser.from_dict(copy.deepcopy(cfg), timestamp='t')
    return config, config.init_metrics()


def test_init_metrics_has_the_similarity_keys_exactly_when_the_option_is_on(tmp_path):
    config, off = _names(tmp_path)
    assert off == _names(tmp_path, image_similarity=False)[1] and not any('similarity' in k for k in off)
    _, on = _names(tmp_path, image_similarity={'bins': 32, 'period': 2})
    C = config['trainer']['no_chains']
    prefixes = ['VI/train/similarity'] + [f'MCMC/chain_{i}/similarity' for i in range(C)] + ['MCMC/similarity_of_mean']
    added = [f'{p}/{k}' for p in prefixes for k in ('MSE', 'NCC', 'MI', 'NMI')]
    assert sorted(on) == sorted(off + added) and len(set(on)) == len(on)
    assert [k for k in on if 'similarity' not in k] == off  # everything else, in today's order
    assert _names(tmp_path, image_similarity=True)[1] == on
    with pytest.raises(ValueError, match='trainer.image_similarity'):
        _names(tmp_path, image_similarity={'bins': 1})


# ---------------------------------------------------------------- the entry points
def test_entry_points_exist_and_refuse_cpu_tensors():
    import inspect

    import torch

    from ir_sgmcmc_amd import _lib as L
    from ir_sgmcmc_amd import ops
    from ir_sgmcmc_amd.utils import calc_image_similarity
    assert list(inspect.signature(ops.image_similarity).parameters) == ['fixed', 'moving', 'mask', 'bins', 'fixed_range',
                                                                        'moving_range', 'want_hist']
    assert list(inspect.signature(calc_image_similarity).parameters) == ['fixed', 'moving', 'mask', 'bins', 'fixed_range',
                                                                         'moving_range']
    assert ops.SIMILARITY_COLUMNS == S.COLUMNS and len(ops.SIMILARITY_COLUMNS) == L.IRS_SIMILARITY_STATS
    im = torch.zeros(1, 1, 4, 4, 4)
    with pytest.raises(L.IrsError):
        ops.image_similarity(im, im, fixed_range=(0.0, 1.0), moving_range=(0.0, 1.0))


def test_arguments_are_validated_on_the_host():
    """everything irs_image_similarity refuses before it touches the device: one fake non-null pointer stands for every array"""
    import ctypes as C

    from ir_sgmcmc_amd import _lib as L
    lib = L.load()
    n = C.c_size_t()
    assert lib.irs_image_similarity_workspace(2, 64, C.byref(n)) == 0 and n.value >= 2 * 64 * 64 * 4
    small = n.value
    assert lib.irs_image_similarity_workspace(L.IRS_MAX_CHAINS, 128, C.byref(n)) == 0
    assert small < n.value <= L.IRS_MAX_CHAINS * 128 * 128 * 4 + 1024 * 9 * 8  # IRS_SIMILARITY_WS_BYTES
    for C_, bins in ((0, 64), (L.IRS_MAX_CHAINS + 1, 64), (1, 1), (1, 129)):
        assert lib.irs_image_similarity_workspace(C_, bins, C.byref(n)) != 0
    assert lib.irs_image_similarity_workspace(1, 64, None) != 0
    p = C.c_void_p(256)
    inf, nan = float('inf'), float('nan')

    def call(fixed=p, Cf=1, moving=p, Cn=2, dims=(4, 4, 4), fr=(0.0, 1.0), mr=(0.0, 1.0), bins=64, stats=p, ws=p, ws_bytes=small):
        return lib.irs_image_similarity(fixed, Cf, moving, Cn, None, *dims, *fr, *mr, bins, None, stats, ws, ws_bytes, None)
    for kw, msg in ((dict(fixed=None), b'bad arguments'), (dict(moving=None), b'bad arguments'), (dict(stats=None), b'bad arguments'),
                    (dict(ws=None), b'bad arguments'), (dict(Cn=0), b'chains'), (dict(Cn=L.IRS_MAX_CHAINS + 1, Cf=1), b'chains'),
                    (dict(Cf=3), b'1 or 2'), (dict(bins=1), b'bins'), (dict(bins=129), b'bins'), (dict(fr=(1.0, 1.0)), b'fixed range'),
                    (dict(fr=(1.0, 0.0)), b'fixed range'), (dict(mr=(0.0, nan)), b'moving range'), (dict(mr=(-inf, 1.0)), b'moving range'),
                    (dict(fr=(-3e38, 3e38)), b'too wide'), (dict(dims=(0, 4, 4)), b'dims'), (dict(dims=(4, 4, -1)), b'dims'),
                    (dict(dims=(1024, 1024, 1024)), b'2^30'), (dict(ws_bytes=small - 1), b'workspace'),
                    (dict(ws=C.c_void_p(264)), b'aligned')):
        assert call(**kw) != 0, kw
        assert msg in lib.irs_last_error(), (kw, lib.irs_last_error())
