"""SGHMC, host side: the numpy restatement of the step (tests/_sghmc.py) against cases worked by hand and against the theory of the
AR(1) process the momentum is without a gradient, the `trainer.sampler` option, the warning for optimiser keys nobody reads, and the
two entry points in the header, the bindings and the export list."""
import copy
import json
import logging
import os
import re

import numpy as np
import pytest
import torch

from ir_sgmcmc_amd import _lib as L
from ir_sgmcmc_amd import sghmc
from tests import _langevin_noise as N
from tests import _sghmc as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def rnd(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(F32)


# ---------------------------------------------------------------- the restatement
def test_constants():
    lr, oma, amp = S.constants(0.5, 1.0, 1.0)
    assert (lr, oma, amp) == (F32(0.5), F32(0.0), F32(1.0))             # amp = sqrt(2 * 1 * 0.5 * 1) = 1 exactly
    assert S.constants(0.4, 0.1, 0.0)[2] == F32(0.0)                    # T = 0: amp = 0
    # oma from the float32 friction, in double: 1 - fl32(0.1) rounded once, not fl32(1) - fl32(0.1) in float32 arithmetic of 0.9
    assert S.constants(0.4, 0.1, 1.0)[1] == F32(1.0 - float(F32(0.1)))
    assert S.constants(0.4, 0.1, 1.0)[2] == F32(np.sqrt(2.0 * float(F32(0.1)) * float(F32(0.4))))


def test_step_by_hand():
    # dyadic numbers: every operation exact.  oma = 0.5, lr = 0.25, amp = sqrt(2 * 0.5 * 0.25 * 4) = 1
    v, m, g, sg, n = (np.array([x], dtype=F32) for x in (3.0, 2.0, 8.0, 0.5, -4.0))
    v1, m1 = S.step(v, m, g, sg, n, lr=0.25, friction=0.5, temperature=4.0)
    assert m1[0] == 0.5 * 2.0 - 0.25 * 8.0 + 1.0 * 0.5 * -4.0 == -3.0 and v1[0] == 0.0
    v1, m1 = S.step(v, m, g, None, n, lr=0.25, friction=0.5, temperature=4.0)     # sigma = 1
    assert m1[0] == -5.0 and v1[0] == -2.0
    v1, m1 = S.step(v, m, g, sg, n, lr=0.25, friction=0.5, temperature=0.0)       # no noise term at all
    assert m1[0] == -1.0 and v1[0] == 2.0


def test_temperature_zero_never_reads_the_noise():
    v, m, g = rnd((64,), 1), rnd((64,), 2), rnd((64,), 3)
    bad = np.full(64, np.nan, dtype=F32)
    v1, m1 = S.step(v, m, g, bad, bad, lr=0.4, friction=0.1, temperature=0.0)
    assert np.isfinite(v1).all() and np.isfinite(m1).all()


def test_friction_one_no_noise_no_momentum_is_the_plain_gradient_step():
    """m' = fsub(fmul(0, 0), fmul(lr, g)) = -fl(lr g) and fadd(v, -x) = fsub(v, x): the step of v <- v - lr g with the product rounded.
    (Where lr is a power of two the product is exact, and the step is also that of a fused multiply-add.)"""
    v, g = rnd((4096,), 4), rnd((4096,), 5)
    for lr in (0.4, 0.0625):
        v1, m1 = S.step(v, np.zeros_like(v), g, None, None, lr=lr, friction=1.0, temperature=0.0)
        prod = F32(lr) * g
        assert np.array_equal(m1, -prod) and np.array_equal(v1, v - prod)
    fma = (v.astype(np.float64) - 0.0625 * g.astype(np.float64)).astype(F32)        # one rounding: exact in double
    assert np.array_equal(S.step(v, np.zeros_like(v), g, None, None, lr=0.0625, friction=1.0, temperature=0.0)[0], fma)


def test_noise_is_scaled_by_sigma_and_added_once():
    v, m, g, n = np.zeros(8, F32), np.zeros(8, F32), np.zeros(8, F32), rnd((8,), 6)
    for sg in (0.5, 1.0, 2.0):
        v1, m1 = S.step(v, m, g, np.full(8, sg, F32), n, lr=0.5, friction=1.0, temperature=1.0)
        assert np.array_equal(m1, F32(sg) * n) and np.array_equal(v1, m1)


def test_ar1_variance_formula_simulated():
    """the momentum without a gradient is AR(1): after n steps from zero its variance is amp^2 (1 - oma^2n) / (1 - oma^2)"""
    M, n, lr, a = 1 << 16, 64, 0.4, 0.5
    rng = np.random.default_rng(7)
    v, m, g = np.zeros(M, F32), np.zeros(M, F32), np.zeros(M, F32)
    for _ in range(n):
        v, m = S.step(v, m, g, None, rng.standard_normal(M).astype(F32), lr=lr, friction=a, temperature=1.0)
    _, oma, amp = S.constants(lr, a, 1.0)
    want = S.ar1_variance(amp, oma, n)
    assert abs(m.astype(np.float64).var() / want - 1.0) < 5.0 * np.sqrt(2.0 / M)
    assert abs(m.astype(np.float64).mean()) < 5.0 * np.sqrt(want / M)
    # its stationary value is lr T / (1 - a / 2): what kinetic_temperature reads as T
    assert S.ar1_variance(amp, oma, 10 ** 6) == pytest.approx(lr / (1.0 - 0.5 * a), rel=1e-6)
    kt = sghmc.kinetic_temperature(torch.from_numpy(m).view(1, -1), None, lr, a)
    assert float(kt[0]) == pytest.approx(m.astype(np.float64).var() * (1.0 - 0.5 * a) / lr, rel=1e-3)


def test_kinetic_temperature_closed_form():
    m = torch.tensor([[1.0, -2.0, 3.0, 0.0], [2.0, 2.0, 2.0, 2.0]])
    sigma = torch.tensor([[1.0, 2.0, 0.5, 1.0], [2.0, 2.0, 2.0, 2.0]])
    kt = sghmc.kinetic_temperature(m, sigma, lr=0.25, friction=0.5)
    assert kt.dtype == torch.float64 and kt.tolist() == [(1.0 + 1.0 + 36.0 + 0.0) / 4 / 0.25 * 0.75, 1.0 / 0.25 * 0.75]
    assert sghmc.kinetic_temperature(m, None, lr=1.0, friction=1.0).tolist() == [14.0 / 4 * 0.5, 4.0 * 0.5]


def test_the_stream_word_separates_the_draws():
    words = N.noise_words(3, 9, 2, (4, 5, 6), stream=S.STREAM)
    assert S.STREAM == 0x484D != N.STREAM and not np.array_equal(words, N.noise_words(3, 9, 2, (4, 5, 6)))
    n, r = S.normals(3, 9, 2, (4, 5, 6))
    assert n.shape == (2, 3, 4, 5, 6) and np.all(np.abs(n) <= r + 1e-12)


# ---------------------------------------------------------------- trainer.sampler
def test_sampler_is_off_unless_asked_for():
    assert sghmc.sampler_options({}) is None
    assert sghmc.sampler_options({'sampler': None}) is None
    assert sghmc.sampler_options({'sampler': {'type': 'SGLD'}}) is None


def test_sampler_values():
    assert sghmc.sampler_options({'sampler': {'type': 'SGHMC'}}) == {'type': 'SGHMC', 'friction': 0.1, 'temperature': 1.0}
    got = sghmc.sampler_options({'sampler': {'type': 'SGHMC', 'friction': 1, 'temperature': 0}})
    assert got == {'type': 'SGHMC', 'friction': 1.0, 'temperature': 0.0} and all(isinstance(got[k], float) for k in ('friction', 'temperature'))
    assert sghmc.sampler_options({'sampler': {'type': 'SGHMC', 'friction': 0.5}})['temperature'] == 1.0
    assert sghmc.sampler_options({'sampler': {'type': 'SGHMC', 'temperature': 0.25}})['friction'] == 0.1


@pytest.mark.parametrize('opt', ['SGHMC', 1, ['SGHMC'], True, {}, {'friction': 0.1}, {'type': 'HMC'}, {'type': 'sghmc'}, {'type': None},
                                 {'type': 'SGHMC', 'frictions': 0.1}, {'type': 'SGHMC', 'lr': 0.1}, {'type': 'SGLD', 'friction': 0.1},
                                 {'type': 'SGLD', 'temperature': 1.0},
                                 {'type': 'SGHMC', 'friction': 0}, {'type': 'SGHMC', 'friction': -0.1}, {'type': 'SGHMC', 'friction': 1.5},
                                 {'type': 'SGHMC', 'friction': float('nan')}, {'type': 'SGHMC', 'friction': '0.1'},
                                 {'type': 'SGHMC', 'friction': True}, {'type': 'SGHMC', 'friction': None},
                                 {'type': 'SGHMC', 'temperature': -1}, {'type': 'SGHMC', 'temperature': float('inf')},
                                 {'type': 'SGHMC', 'temperature': float('nan')}, {'type': 'SGHMC', 'temperature': 'hot'},
                                 {'type': 'SGHMC', 'temperature': False}])
def test_sampler_refusals(opt):
    with pytest.raises(ValueError, match='trainer.sampler'):
        sghmc.sampler_options({'sampler': opt})


def _trainer(tmp_path, name, sampler=None, optimizer_args=None):
    from ir_sgmcmc_amd.parse_config import ConfigParser
    from ir_sgmcmc_amd.trainer import Trainer
    cfg = json.load(open(os.path.join(ROOT, 'configs', name)))
    cfg['trainer']['save_dir'] = str(tmp_path)
    cfg['data_loader']['args']['dims'] = [16, 16, 16]
    if sampler is not None:
        cfg['trainer']['sampler'] = sampler
    if optimizer_args is not None:
        cfg['optimizer_SG_MCMC']['args'] = optimizer_args
    config = ConfigParser.from_dict(copy.deepcopy(cfg), timestamp='t')
    dl = config.init_data_loader()
    tm, rm = config.init_transformation_and_registration_modules()
    return Trainer(config, dl, config.init_losses(), tm, rm, [], device='cpu')


def test_the_trainer_reads_the_option_and_the_config(tmp_path):
    t = _trainer(tmp_path / 'a', 'synthetic_ssd_l2_128_sghmc.json')
    assert t.sampler_options == {'type': 'SGHMC', 'friction': 0.1, 'temperature': 1.0}
    ec = t._engine_config()
    assert (ec.sampler, ec.sghmc_friction, ec.sghmc_temperature) == ('SGHMC', 0.1, 1.0)
    assert t.ess_options is not None and t.truth_options is not None
    # its SGLD twin: the truth config, and the same config with the sampler named
    for twin in (_trainer(tmp_path / 'b', 'synthetic_ssd_l2_128_truth.json'),
                 _trainer(tmp_path / 'c', 'synthetic_ssd_l2_128_sghmc.json', sampler={'type': 'SGLD'})):
        assert twin.sampler_options is None and twin._engine_config().sampler == 'SGLD'
    with pytest.raises(ValueError, match='friction'):
        _trainer(tmp_path / 'd', 'synthetic_ssd_l2_128_sghmc.json', sampler={'type': 'SGHMC', 'friction': 2})
    # the new config is the truth config plus the diagnostics and the sampler, nothing else
    new = json.load(open(os.path.join(ROOT, 'configs', 'synthetic_ssd_l2_128_sghmc.json')))
    old = json.load(open(os.path.join(ROOT, 'configs', 'synthetic_ssd_l2_128_truth.json')))
    assert new['trainer'].pop('sampler')['type'] == 'SGHMC' and new['trainer'].pop('convergence_diagnostics')['ess'] is True
    assert new.pop('name') != old.pop('name') and new == old


class _Collect(logging.Handler):
    def __init__(self):
        super().__init__(logging.WARNING)
        self.messages = []

    def emit(self, record):
        self.messages.append(record.getMessage())


def _warnings_of(build):
    """the warnings about the optimiser's keys that building a trainer leaves on the package's logger"""
    handler = _Collect()

    logger = logging.getLogger('default')
    original = logger.callHandlers  # (the logging set-up of a new config may replace handlers: listen in front of them instead)

    def call(record):
        handler.handle(record) if record.levelno >= logging.WARNING else None
        return original(record)
    logger.callHandlers = call
    try:
        trainer = build()
    finally:
        del logger.callHandlers
    return trainer, [m for m in handler.messages if 'optimizer_SG_MCMC' in m]


def test_extra_optimiser_keys_are_named_once(tmp_path):
    assert sghmc.extra_optimizer_keys({'type': 'SGD', 'args': {'lr': 0.4}}) == []
    assert sghmc.extra_optimizer_keys({'type': 'SGD'}) == []
    assert sghmc.extra_optimizer_keys({'type': 'SGD', 'args': {'momentum': 0.9, 'lr': 0.4, 'dampening': 0}}) == ['dampening', 'momentum']
    t, got = _warnings_of(lambda: _trainer(tmp_path / 'a', 'synthetic_ssd_l2_128_truth.json', optimizer_args={'lr': 0.4, 'momentum': 0.9}))
    assert len(got) == 1 and "['momentum']" in got[0] and 'ignored' in got[0], got
    assert t._engine_config().lr == 0.4  # what they do has not changed: nothing
    _, got = _warnings_of(lambda: _trainer(tmp_path / 'b', 'synthetic_ssd_l2_128_truth.json'))
    assert got == []


# ---------------------------------------------------------------- the C ABI
def test_header_bindings_and_export_list():
    header = open(os.path.join(ROOT, 'include', 'irsgmcmc.h')).read()
    exports = open(os.path.join(ROOT, 'ir_sgmcmc_amd', 'csrc', 'exports.map')).read()
    assert re.search(r'global:\s*irs_\*;', exports) and re.search(r'local:\s*\*;', exports)
    for name, nargs in (('irs_sghmc_set', 4), ('irs_sghmc_update', 15)):
        decl = re.search(r'^int ' + name + r'\(([^;]*)\);', header, re.M | re.S)
        assert decl, name
        assert len(decl.group(1).split(',')) == nargs == len(L.SIGNATURES[name])
        assert name.startswith('irs_')  # what the export list lets out
    assert L.SIGNATURES['irs_sghmc_update'][-3:-1] == [L.C.c_uint64, L.C.c_uint64]
    so = os.path.join(ROOT, 'ir_sgmcmc_amd', 'csrc', 'libirsgmcmc.so')
    if os.path.isfile(so):
        lib = L.C.CDLL(so)
        assert hasattr(lib, 'irs_sghmc_set') and hasattr(lib, 'irs_sghmc_update')
