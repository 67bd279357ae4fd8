"""The host side of the residual model check, without a GPU: residual_check.residual_fit against the restatement of
tests/_residual_check.py and against closed forms, mixture_terms for both data losses, the trainer.residual_check option, the
metric names, the CSV layout, and what the three operator wrappers hand to the C ABI (through a recording stand-in of the
library, as tests/test_ops_calls_host.py does for ops.py)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from ir_sgmcmc_amd import _lib as L
from ir_sgmcmc_amd import residual_check as R
from ir_sgmcmc_amd.diagnostics import (RESIDUAL_METRICS, residual_check_metric_names, residual_check_options, residual_map_summary,
                                       residual_metrics)
from ir_sgmcmc_amd.logger import residual_histogram_rows
from ir_sgmcmc_amd.model.loss import GMM, SSD
from tests import _residual_check as S

STD, PI = (0.05, 0.2), (0.7, 0.3)


# ---------------------------------------------------------------- residual_fit
@pytest.mark.parametrize('bins,h,std,pi', [(32, 0.8, STD, PI), (2, 0.3, STD, PI), (37, 0.1, (0.03, 0.08, 0.5), (0.2, 0.5, 0.3)),
                                           (512, 1.0, (0.1,), (1.0,))])
def test_fit_against_the_restatement(bins, h, std, pi):
    z = S.spoil(S.draw_mixture((9, 10, 11), 2, std, pi, seed=bins), None, h, seed=1)
    hist, counts, sums = S.reference_histogram(z, None, h, bins)
    got = R.residual_fit(torch.from_numpy(hist), torch.from_numpy(counts), torch.from_numpy(sums), h, std, pi)
    assert len(got) == 2
    for c in range(2):
        want = S.reference_fit(hist[c], counts[c], sums[c], h, std, pi)
        assert list(got[c]) == list(R.FIT_KEYS) == list(S.FIT_KEYS) and got[c]['n'] == want['n'] == int(counts[c, 0]) > 0
        for k in R.FIT_KEYS:  # the same float64 formulas, summed in another order: a few ulp of the largest term
            assert got[c][k] == pytest.approx(want[k], rel=1e-12, abs=1e-14), k
    one = R.residual_fit(hist[0], counts[0], sums[0], h, std, pi)  # one chain in, one dict out
    assert one == got[0]


def test_closed_forms():
    # one bin per half under a symmetric model: p = 1/2, 1/2
    p, F = R.model_probabilities(0.4, 2, STD, PI)
    assert p.tolist() == [0.5, 0.5] and F[1] == 0.5
    fit = R.residual_fit(np.array([30, 10]), np.array([40, 0, 0]), np.array([0.0, 1.0, 1.0, 0.5]), 0.4, STD, PI)
    assert fit['tv'] == 0.25 and fit['ks'] == 0.25 and fit['chi2'] == pytest.approx(0.25)
    assert fit['kl'] == pytest.approx(0.75 * math.log(1.5) + 0.25 * math.log(0.5))
    # the bins of a model sum to 1 and the end bins hold the tails
    p, _ = R.model_probabilities(0.1, 16, STD, PI)
    assert p.sum() == pytest.approx(1.0, abs=1e-15) and p[0] == pytest.approx(p[-1], rel=1e-13) and p[0] > p[1]
    # one component: kurtosis 3, std sigma, the tail of a Gaussian
    fit = R.residual_fit(np.array([1, 1]), np.array([2, 0, 0]), np.array([0.0, 2.0, 2.0, 1.0]), 2.0, [0.5], [1.0])
    assert fit['kurtosis_model'] == 3.0 and fit['std_model'] == 0.5 and fit['tail_model'] == math.erfc(4.0 / math.sqrt(2.0))
    assert fit['kurtosis'] == 1.0 and fit['std'] == 1.0 and fit['mean'] == 0.0
    # a model with no mass where a sample fell: KL is +inf, chi2 skips the bin
    fit = R.residual_fit(np.array([0, 1, 0, 0, 0, 0, 0, 0]), np.array([1, 0, 0]), np.array([-60.0, 3600.0, 1.296e7, 60.0]), 100.0,
                         [1e-3], [1.0])
    assert fit['kl'] == math.inf and math.isfinite(fit['chi2']) and fit['tv'] == 1.0
    # nothing took part
    fit = R.residual_fit(np.zeros(8, np.int64), np.array([0, 5, 0]), np.array([0.0, 0.0, 0.0, -math.inf]), 1.0, STD, PI)
    assert fit['n'] == 0 and all(math.isnan(fit[k]) for k in R.FIT_KEYS if k != 'n')
    with pytest.raises(ValueError, match='proportions'):
        R.residual_fit(np.zeros(8), np.zeros(3), np.zeros(4), 1.0, [1.0, 2.0], [1.0])


def test_the_restatement_alone_tells_the_right_mixture_from_the_wrong_one():
    """the statistical case of the GPU test, on the host: 2 n KL is chi-square with B - 1 degrees of freedom under the model"""
    B, h, shape = 32, 0.8, (17, 16, 65)
    z = S.draw_mixture(shape, 1, STD, PI, seed=7)
    hist, counts, sums = S.reference_histogram(z, None, h, B)
    n = int(counts[0, 0])
    right = S.reference_fit(hist[0], counts[0], sums[0], h, STD, PI)
    wrong = S.reference_fit(hist[0], counts[0], sums[0], h, [2 * s for s in STD], PI)
    print(f'n = {n}: KL against the mixture drawn from {right["kl"]:.3e} (bound {5 * (B - 1) / (2 * n):.3e}), against the doubled '
          f'scales {wrong["kl"]:.3e}')
    assert right['kl'] < 5 * (B - 1) / (2 * n) and wrong['kl'] > 0.1
    assert right['std'] / right['std_model'] == pytest.approx(1.0, abs=0.05) and wrong['std'] / wrong['std_model'] < 0.6


# ---------------------------------------------------------------- mixture_terms
def test_mixture_terms():
    g = GMM(4, 1)
    with torch.no_grad():
        g.log_std.copy_(torch.tensor([-3.0, -2.0, -1.0, 0.5]))
        g.logits.copy_(torch.tensor([0.3, -0.2, 1.0, 0.0]))
    std, pi, lw, inv = R.mixture_terms(g)
    assert [type(x) for x in (std, pi, lw, inv)] == [list] * 4 and all(isinstance(v, float) for x in (std, pi, lw, inv) for v in x)
    log_pi = g.log_proportions.detach().double()  # the model's own, with its + 1e-2
    assert pi == pytest.approx(torch.exp(log_pi).tolist(), rel=1e-15) and sum(pi) == pytest.approx(1.0, abs=1e-6)
    assert std == pytest.approx([math.exp(x) for x in g.log_std.detach().tolist()], rel=1e-15)  # of the float32 parameter, in float64
    assert std == pytest.approx(g.scales.detach().tolist(), rel=1e-6)
    for k in range(4):
        assert lw[k] == pytest.approx(float(log_pi[k]) - float(g.log_std.detach()[k]) - 0.5 * math.log(2 * math.pi), rel=1e-14)
        assert inv[k] == pytest.approx(1.0 / std[k], rel=1e-14)
    # the density these terms give is the model's own log_pdf
    z = torch.tensor([0.0, 0.01, -0.3, 2.0])
    mine = -S.nll(z.numpy(), np.array(lw), np.array(inv))
    assert mine == pytest.approx(g.log_pdf(z).detach().reshape(-1).double().numpy(), rel=1e-5, abs=1e-5)
    std, pi, lw, inv = R.mixture_terms(SSD(0.25))
    assert (std, pi, inv) == ([0.25], [1.0], [4.0]) and lw == [pytest.approx(-math.log(0.25) - 0.5 * math.log(2 * math.pi))]
    with pytest.raises(TypeError, match='neither'):
        R.mixture_terms(torch.nn.Identity())


# ---------------------------------------------------------------- the option, the metric names, the CSV
BASE = {'log_period_MCMC': 10, 'no_samples_MCMC': 40, 'no_chains': 2}


def test_option_parsing():
    assert residual_check_options(BASE) is None and residual_check_options({**BASE, 'residual_check': False}) is None
    assert residual_check_options({**BASE, 'residual_check': None}) is None
    assert residual_check_options({**BASE, 'residual_check': True}) == {'period': 10, 'bins': 128, 'range': None, 'nll_map': True,
                                                                        'save': True}
    opt = {'bins': 64, 'range': 2, 'period': 5, 'nll_map': False, 'save': False}
    assert residual_check_options({**BASE, 'residual_check': opt}) == {'period': 5, 'bins': 64, 'range': 2.0, 'nll_map': False,
                                                                       'save': False}
    assert residual_check_options({**BASE, 'residual_check': {}})['bins'] == 128


@pytest.mark.parametrize('opt,message', [
    ({'colour': 1}, r"trainer.residual_check: unknown keys \['colour'\]; known: \['bins', 'range', 'period', 'nll_map', 'save'\]"),
    ('yes', r'trainer.residual_check must be true, false or \{"bins": B, "range": h, "period": P, "nll_map": bool, "save": bool\}'),
    ({'bins': 64.0}, 'trainer.residual_check.bins must be an integer, got 64.0'),
    ({'bins': True}, 'trainer.residual_check.bins must be an integer, got True'),
    ({'bins': 1}, r'trainer.residual_check: bins must be in 2 \.\. 512, got 1'),
    ({'bins': 513}, r'trainer.residual_check: bins must be in 2 \.\. 512, got 513'),
    ({'range': 0}, r'trainer.residual_check.range must be a finite number > 0, got 0'),
    ({'range': float('inf')}, r'trainer.residual_check.range must be a finite number > 0, got inf'),
    ({'range': '1'}, r"trainer.residual_check.range must be a finite number > 0, got '1'"),
    ({'period': 2.0}, 'trainer.residual_check.period must be an integer, got 2.0'),
    ({'period': 0}, 'trainer.residual_check: the period must be >= 1, got 0'),
    ({'period': 41}, 'trainer.residual_check: no_samples_MCMC = 40 with period 41 records no step'),
    ({'nll_map': 1}, 'trainer.residual_check.nll_map must be true or false, got 1'),
    ({'save': 'no'}, "trainer.residual_check.save must be true or false, got 'no'")])
def test_option_refusals(opt, message):
    with pytest.raises(ValueError, match=message):
        residual_check_options({**BASE, 'residual_check': opt})


def test_metric_names_and_summaries():
    keys = ['KL', 'TV', 'KS', 'chi2', 'tail', 'std_ratio', 'kurtosis_ratio']
    assert [k for k, _ in RESIDUAL_METRICS] == keys
    on = residual_check_options({**BASE, 'residual_check': True})
    names = residual_check_metric_names(on, 2)
    prefixes = ['VI/train/residuals', 'MCMC/chain_0/residuals', 'MCMC/chain_1/residuals', 'MCMC/residuals']
    assert names == [f'{p}/{k}' for p in prefixes for k in keys] + ['MCMC/residuals/nll_mean', 'MCMC/residuals/nll_max']
    with_vi = residual_check_metric_names(on, 1, vi=True)
    assert [n for n in with_vi if n.startswith('VI/residuals/')] == [f'VI/residuals/{k}' for k in keys]
    no_map = residual_check_metric_names({**on, 'nll_map': False}, 2)
    assert no_map == names[:-2]
    row = dict.fromkeys(R.FIT_KEYS, 0.5) | {'std': 0.3, 'std_model': 0.2, 'kurtosis': 6.0, 'kurtosis_model': 3.0}
    assert residual_metrics(row) == {'KL': 0.5, 'TV': 0.5, 'KS': 0.5, 'chi2': 0.5, 'tail': 0.5, 'std_ratio': 0.3 / 0.2,
                                     'kurtosis_ratio': 2.0}
    assert all(math.isnan(v) for v in residual_metrics(dict.fromkeys(R.FIT_KEYS, math.nan)).values())
    assert residual_map_summary([10, 2], [16.0, 5.0], 6) == {'records': 6, 'voxels': 10, 'empty_voxels': 2, 'nll_mean': 2.0,
                                                             'nll_max': 5.0}
    empty = residual_map_summary([3, 3], [0.0, -math.inf], 2)
    assert math.isnan(empty['nll_mean']) and math.isnan(empty['nll_max'])
    from ir_sgmcmc_amd.parse_config import ConfigParser  # the config's metric list takes the names in
    import json
    import os
    cfg = json.load(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'configs',
                                      'synthetic_gmm_lognormal.json')))
    plain = ConfigParser.from_dict(json.loads(json.dumps(cfg)), timestamp='t').init_metrics()
    cfg['trainer']['residual_check'] = True
    assert ConfigParser.from_dict(cfg, timestamp='t').init_metrics() == plain + names


def test_csv_layout():
    hist = np.array([[1, 2, 3, 4], [0, 5, 0, 7]])
    p, _ = R.model_probabilities(1.0, 4, STD, PI)
    header, rows = residual_histogram_rows(R.bin_edges(1.0, 4), torch.from_numpy(hist), p)
    assert header == ['bin_lo', 'bin_hi', 'count_chain_0', 'count_chain_1', 'count', 'model_probability']
    assert [r[:5] for r in rows] == [['-1.0', '-0.5', '1', '0', '1'], ['-0.5', '0.0', '2', '5', '7'], ['0.0', '0.5', '3', '0', '3'],
                                     ['0.5', '1.0', '4', '7', '11']]
    assert [float(r[5]) for r in rows] == p.tolist()


# ---------------------------------------------------------------- the wrappers, through a recording stand-in of the library
class Token:
    def __init__(self, tensor):
        self.tensor = tensor


class Recorder:
    def __init__(self):
        self.calls = []

    def load(self, path=None):
        return self

    @staticmethod
    def dev_ptr(tensor, dtype=None, allow_none=False):
        if tensor is None:
            if allow_none:
                return None
            raise L.IrsError('required tensor is None')
        if dtype is not None and tensor.dtype != dtype:
            raise L.IrsError(f'expected {dtype}, got {tensor.dtype}')
        if not tensor.is_contiguous():
            raise L.IrsError('tensor must be contiguous')
        return Token(tensor)

    @staticmethod
    def stream_ptr():
        return 'stream'

    def __getattr__(self, name):
        if name not in L.SIGNATURES:
            raise AttributeError(name)

        def fn(*args):
            argtypes = L.SIGNATURES[name]
            assert len(args) == len(argtypes), f'{name}: {len(args)} arguments for {len(argtypes)} parameters'
            row = []
            for i, (a, ty) in enumerate(zip(args, argtypes)):
                if isinstance(a, Token) or (isinstance(a, str) and a == 'stream'):
                    assert ty is C.c_void_p, f'{name}: argument {i} is a device pointer, the header has {ty.__name__}'
                    row.append(a if isinstance(a, str) else (tuple(a.tensor.shape), a.tensor.dtype, a.tensor.data_ptr()))
                else:
                    ty.from_param(a)  # TypeError / ArgumentError where ctypes would refuse the value
                    row.append(list(a) if isinstance(a, C.Array) else a)
            self.calls.append((name, row))
            return 0
        return fn


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(L, 'load', r.load)
    monkeypatch.setattr(L, 'dev_ptr', r.dev_ptr)
    monkeypatch.setattr(L, 'stream_ptr', r.stream_ptr)
    return r


Cn, D, H, W = 2, 4, 5, 6
f32 = torch.float32


def test_histogram_wrapper(rec):
    z, mask = torch.zeros(Cn, 1, D, H, W), torch.ones(1, 1, D, H, W, dtype=torch.bool)
    out = R.residual_histogram(z, mask, 0.5, 37)
    assert list(out) == ['hist', 'counts', 'sums']
    assert [(tuple(t.shape), t.dtype) for t in out.values()] == [((Cn, 37), torch.int64), ((Cn, 3), torch.int64), ((Cn, 4), torch.float64)]
    (name, a), = rec.calls
    assert name == 'irs_residual_histogram'
    assert a[0] == ((Cn, 1, D, H, W), f32, z.data_ptr()) and a[1] == Cn and a[2][:2] == ((1, 1, D, H, W), torch.uint8)
    assert a[3:8] == [D, H, W, 0.5, 37] and [x[2] for x in a[8:11]] == [out[k].data_ptr() for k in out] and a[11] == 0
    assert a[12][0] == (L.IRS_RESIDUAL_WS_BYTES,) and a[13] == L.IRS_RESIDUAL_WS_BYTES and a[14] == 'stream'
    # the state goes back in; no mask is a NULL
    again = R.residual_histogram(z, None, 0.5, 37, **out, records_before=Cn)
    assert all(again[k] is out[k] for k in out) and rec.calls[1][1][2] is None and rec.calls[1][1][11] == Cn
    for kw, message in (({'records_before': 2}, "records_before = 2 needs the state of the earlier calls; \\['hist', 'counts', 'sums'\\]"),
                        ({'hist': torch.zeros(Cn, 36, dtype=torch.int64)}, r'hist must be a \(2, 37\) torch.int64 tensor'),
                        ({'sums': torch.zeros(Cn, 4)}, r'sums must be a \(2, 4\) torch.float64 tensor')):
        with pytest.raises(L.IrsError, match=message):
            R.residual_histogram(z, None, 0.5, 37, **kw)
    with pytest.raises(L.IrsError, match='bins must be an integer'):
        R.residual_histogram(z, None, 0.5, 37.0)
    with pytest.raises(L.IrsError, match=r'mask must be a bool / uint8 \(1,1,4,5,6\) volume'):
        R.residual_histogram(z, torch.ones(Cn, 1, D, H, W, dtype=torch.bool), 0.5, 37)
    with pytest.raises(L.IrsError, match='expected a'):
        R.residual_histogram(z[:, 0], None, 0.5, 37)
    assert len(rec.calls) == 2


def test_nll_wrappers(rec):
    z = torch.zeros(Cn, 1, D, H, W)
    mean, count = torch.zeros(D, H, W), torch.zeros(D, H, W, dtype=torch.int32)
    assert R.residual_nll_update(z, [0.5, -1.0, 2.0], np.array([1.0, 2.0, 4.0]), mean, count, 4) is None
    (name, a), = rec.calls
    assert name == 'irs_residual_nll_update' and a[1:5] == [Cn, D, H, W] and a[5] == [0.5, -1.0, 2.0] and a[6] == [1.0, 2.0, 4.0]
    assert a[7] == 3 and a[8] == ((D, H, W), f32, mean.data_ptr()) and a[9] == ((D, H, W), torch.int32, count.data_ptr())
    assert a[10] == 4 and a[11] == 'stream'
    with pytest.raises(L.IrsError, match='inv_std must hold 3 numbers, got 2'):
        R.residual_nll_update(z, [0.5, -1.0, 2.0], [1.0, 2.0], mean, count, 0)
    with pytest.raises(L.IrsError, match=r'count must be a \(4, 5, 6\) torch.int32 tensor'):
        R.residual_nll_update(z, [0.0], [1.0], mean, count.long(), 0)
    R.residual_nll_update(z, [], [], mean, count, 0)  # K = 0 reaches the library, which refuses it
    assert rec.calls[1][1][7] == 0
    isum, fsum = R.residual_nll_finalize(mean, count, torch.ones(D, H, W, dtype=torch.uint8))
    assert (tuple(isum.shape), isum.dtype, tuple(fsum.shape), fsum.dtype) == ((2,), torch.int64, (2,), torch.float64)
    name, a = rec.calls[2]
    assert name == 'irs_residual_nll_finalize' and a[2][:2] == ((D, H, W), torch.uint8) and a[3:6] == [D, H, W]
    assert a[8][0] == (L.IRS_RESIDUAL_MAP_WS_BYTES,) and a[9] == L.IRS_RESIDUAL_MAP_WS_BYTES
    with pytest.raises(L.IrsError, match=r'mean must have shape \(D,H,W\)'):
        R.residual_nll_finalize(mean[None], count)
