"""The ASD metric's host surface (calc_metrics, the metric names, argument checks): no GPU needed."""
import copy
import json
import os

import pytest
import torch

from ir_sgmcmc_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_calc_metrics_is_exported():
    from ir_sgmcmc_amd.utils import calc_metrics
    import inspect
    assert list(inspect.signature(calc_metrics).parameters) == ['seg_fixed', 'seg_moving', 'structures_dict', 'spacing', 'GPU',
                                                                'no_samples']


def test_init_metrics_names_asd_per_chain(tmp_path):
    from ir_sgmcmc_amd.parse_config import ConfigParser
    cfg = json.load(open(os.path.join(ROOT, 'configs', 'synthetic_gmm_lognormal.json')))
    cfg['trainer']['save_dir'] = str(tmp_path)
    config = ConfigParser.from_dict(copy.deepcopy(cfg), timestamp='t')
    names = config.init_metrics()
    for i in range(cfg['trainer']['no_chains']):
        for s in config.structures_dict:
            assert f'MCMC/chain_{i}/ASD/{s}' in names and f'MCMC/chain_{i}/DSC/{s}' in names


def test_label_surface_distance_refuses_cpu_tensors():
    from ir_sgmcmc_amd import ops
    seg = torch.zeros(1, 1, 8, 8, 8, dtype=torch.int16)
    with pytest.raises(L.IrsError):
        ops.label_surface_distance(seg, seg, [10, 16], (1.0, 1.0, 1.0))


def test_surface_distance_workspace_validates_boxes():
    """the boxes come back from the device; the host checks them before they size anything"""
    import ctypes as C
    lib = L.load()
    n = C.c_size_t()
    ok = (C.c_int32 * 12)(1, 2, 3, 4, 5, 6, 2**31 - 1, 2**31 - 1, 2**31 - 1, -1, -1, -1)  # one box, one empty pair
    assert lib.irs_surface_distance_workspace(ok, 2, 8, 8, 8, C.byref(n)) == 0
    assert n.value >= 4 * 4 * 4 * 9
    bad = (C.c_int32 * 6)(0, 0, 0, 8, 1, 1)  # z beyond the volume
    assert lib.irs_surface_distance_workspace(bad, 1, 8, 8, 8, C.byref(n)) != 0
    assert b'out of the volume' in lib.irs_last_error()
