"""The Hausdorff metrics' host surface: the CPU restatement against numpy's inverted-CDF percentile, the trainer option and
the metric names.  No GPU needed."""
import copy
import json
import os

import numpy as np
import pytest

from tests import _hausdorff as HD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('dims', [(23, 37, 50), (9, 11, 150)])
def test_restatement_is_numpys_inverted_cdf(dims):
    f, m = HD.fuzz_maps(dims, 1, 1)
    sets, strict = 0, 0
    for lab in HD.LABELS:
        a, b = HD.contour(f[0, 0] == lab), HD.contour(m[0, 0] == lab)
        if not a.any() or not b.any():
            continue
        for src, dst in ((a, b), (b, a)):
            d2 = HD.nearest_d2(src, dst, (1.0, 1.0, 1.0))
            for q in (50, 95, 99.5, 100):
                assert HD.directed_percentile(d2, q) == np.percentile(d2, q, method='inverted_cdf'), (lab, q)
            assert HD.directed_percentile(d2, 100) == d2.max()
            sets += 1
            strict += HD.directed_percentile(d2, 95) < d2.max()
    assert sets >= 10 and strict >= sets // 3  # the inputs are not degenerate: HD95 < HD in many directed sets


def test_order_index_rule():
    assert HD.order_index(95, 1) == 0 and HD.order_index(100, 1) == 0
    assert HD.order_index(95, 20) == 18 and HD.order_index(95, 21) == 19 and HD.order_index(100, 20) == 19
    assert HD.order_index(1e-9, 1000) == 0 and HD.order_index(0.1, 1000) == 0 and HD.order_index(0.1, 1001) == 1
    assert HD.order_index(50, 4) == 1 and HD.order_index(50, 5) == 2


def test_options_helper_parses():
    from ir_sgmcmc_amd.diagnostics import hausdorff_metric_names, hausdorff_options
    assert hausdorff_options({}) is None
    assert hausdorff_options({'hausdorff': False}) is None and hausdorff_options({'hausdorff': None}) is None
    assert hausdorff_options({'hausdorff': True}) == {'percentiles': (95.0,)}
    assert hausdorff_options({'hausdorff': {}}) == {'percentiles': (95.0,)}
    opt = hausdorff_options({'hausdorff': {'percentiles': [95, 99.5]}})
    assert opt == {'percentiles': (95.0, 99.5)}
    assert hausdorff_metric_names(opt) == ['HD', 'HD95', 'HD99.5']
    assert hausdorff_options({'hausdorff': {'percentiles': []}}) == {'percentiles': ()}
    assert hausdorff_options({'hausdorff': {'percentiles': [1, 50, 95, 100]}})['percentiles'] == (1.0, 50.0, 95.0, 100.0)


@pytest.mark.parametrize('bad', [1, 'yes', [95], {'percentile': [95]}, {'percentiles': 95}, {'percentiles': [0]},
                                 {'percentiles': [100.5]}, {'percentiles': [95, 95]}, {'percentiles': [99, 95]},
                                 {'percentiles': [True]}, {'percentiles': ['95']}, {'percentiles': [float('nan')]},
                                 {'percentiles': [10, 20, 30, 40, 50]}])
def test_options_helper_rejects(bad):
    from ir_sgmcmc_amd.diagnostics import hausdorff_options
    with pytest.raises(ValueError, match='trainer.hausdorff'):
        hausdorff_options({'hausdorff': bad})


def _names(tmp_path, **trainer_over):
    from ir_sgmcmc_amd.parse_config import ConfigParser
    cfg = json.load(open(os.path.join(ROOT, 'configs', 'synthetic_gmm_lognormal.json')))
    cfg['trainer'].update(save_dir=str(tmp_path), **trainer_over)
    config = ConfigParser.from_dict(copy.deepcopy(cfg), timestamp='t')
    return config, config.init_metrics()


def test_init_metrics_has_the_hd_keys_exactly_when_the_option_is_on(tmp_path):
    config, off = _names(tmp_path)
    assert off == _names(tmp_path, hausdorff=False)[1] and not any('/HD' in k for k in off)
    _, on = _names(tmp_path, hausdorff={'percentiles': [95, 99]})
    C = config['trainer']['no_chains']
    added = [f'MCMC/chain_{i}/{k}/{s}' for i in range(C) for k in ('HD', 'HD95', 'HD99') for s in config.structures_dict]
    assert sorted(on) == sorted(off + added) and len(set(on)) == len(on)
    assert [k for k in on if '/HD' not in k] == off  # everything else, in today's order
    with pytest.raises(ValueError, match='trainer.hausdorff'):
        _names(tmp_path, hausdorff={'percentiles': [0]})


def test_entry_points_exist_and_refuse_cpu_tensors():
    import inspect

    import torch

    from ir_sgmcmc_amd import _lib as L
    from ir_sgmcmc_amd import ops
    from ir_sgmcmc_amd.utils import calc_surface_metrics
    assert list(inspect.signature(calc_surface_metrics).parameters) == ['seg_fixed', 'seg_moving', 'structures_dict', 'spacing',
                                                                        'percentiles', 'no_samples']
    seg = torch.zeros(1, 1, 8, 8, 8, dtype=torch.int16)
    with pytest.raises(L.IrsError):
        ops.label_hausdorff_distance(seg, seg, [10, 16], (1.0, 1.0, 1.0))


def test_workspace_and_arguments_are_validated_on_the_host():
    """everything the C entry points refuse before they touch the device"""
    import ctypes as C

    from ir_sgmcmc_amd import _lib as L
    lib = L.load()
    n, n_asd = C.c_size_t(), C.c_size_t()
    ok = (C.c_int32 * 12)(1, 2, 3, 4, 5, 6, 2**31 - 1, 2**31 - 1, 2**31 - 1, -1, -1, -1)  # one box, one empty pair
    assert lib.irs_surface_distance_workspace(ok, 2, 8, 8, 8, C.byref(n_asd)) == 0
    assert lib.irs_hausdorff_workspace(ok, 2, 0, 8, 8, 8, C.byref(n)) == 0 and n.value >= n_asd.value
    assert lib.irs_hausdorff_workspace(ok, 2, 4, 8, 8, 8, C.byref(n)) == 0 and n.value >= n_asd.value + 4 * 4 * 4 * 256 * 4
    for Q in (-1, L.IRS_HAUSDORFF_MAX_PERCENTILES + 1):
        assert lib.irs_hausdorff_workspace(ok, 2, Q, 8, 8, 8, C.byref(n)) != 0
        assert b'percentiles' in lib.irs_last_error()
    bad = (C.c_int32 * 6)(0, 0, 0, 8, 1, 1)  # z beyond the volume
    assert lib.irs_hausdorff_workspace(bad, 1, 1, 8, 8, 8, C.byref(n)) != 0
    assert b'out of the volume' in lib.irs_last_error()
    # the distance call: one fake non-null pointer stands for every device array; all of these return before a launch
    p = C.c_void_p(256)
    lab = (C.c_int32 * 2)(10, 16)
    sp = (C.c_float * 3)(1.0, 1.0, 1.0)

    def call(spacing=sp, pct=(95.0,), ws_bytes=n.value, hd=p, hd_pct=p, Q=None):
        arr = (C.c_double * max(len(pct), 1))(*pct)
        return lib.irs_label_hausdorff_distance(p, 1, p, lab, 2, spacing, ok, p, ws_bytes, arr, len(pct) if Q is None else Q, p, p,
                                                hd, hd_pct, 1, 8, 8, 8, None)
    for kw, msg in ((dict(pct=(0.0,)), b'(0, 100]'), (dict(pct=(101.0,)), b'(0, 100]'), (dict(pct=(95.0, 95.0)), b'increase'),
                    (dict(pct=(float('nan'),)), b'(0, 100]'), (dict(Q=5), b'percentiles'), (dict(Q=-1), b'percentiles'),
                    (dict(spacing=(C.c_float * 3)(1.0, 0.0, 1.0)), b'spacing'),
                    (dict(spacing=(C.c_float * 3)(1.0, float('inf'), 1.0)), b'spacing'), (dict(ws_bytes=16), b'workspace'),
                    (dict(hd=None), b'bad arguments'), (dict(hd_pct=None), b'hd_pct')):
        assert call(**kw) != 0, kw
        assert msg in lib.irs_last_error(), (kw, lib.irs_last_error())
