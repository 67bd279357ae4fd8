"""The posterior comparison on the CPU: the known answers against the numpy restatement, the host build of the per-voxel
arithmetic (tests/csrc/compare_check.cpp compiles ir_sgmcmc_amd/csrc/compare_device.h, the header the kernel compiles) against
closed forms, invariants and the restatement over the GPU test's own cases, the option's parsing, the metric names and the
summary.  The program is built with the address and undefined-behaviour sanitizers where the compiler has them; it is
stand-alone, nothing of it is loaded into Python.

The constants C_B and C_J of tests/_posterior_comparison.py come from `test_host_build_matches_the_restatement`, which prints
the worst ratios it measures."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from ir_sgmcmc_amd.diagnostics import COMPARISON_METRICS, posterior_comparison_options
from ir_sgmcmc_amd.posterior_comparison import comparison_summary
from tests import _posterior_comparison as P


# ---------------------------------------------------------------- the restatement itself
def known_ref():
    ma, Ma, mb, Mb, which = P.known_states()
    return P.compare_np(ma, Ma, P.KNOWN_N[0], mb, Mb, P.KNOWN_N[1], (1.0, 1.0, 1.0)), which, (ma, Ma, mb, Mb)


def test_known_answers_against_the_restatement():
    ref, which, _ = known_ref()
    assert ref['finite'].all()
    planes = {k: ref[k].astype(np.float32) for k in P.PLANES}
    P.check_known(planes, ref['floored'], which)
    same = which == list(P.KNOWN).index('identical')
    assert (ref['shift'][same] == 0).all() and (ref['log_std_ratio'][same] == 0).all()
    # the restatement in float64, closer than float32 storage allows: bures^2 and jeffreys of the table
    for idx, row in enumerate(P.KNOWN.values()):
        at = which == idx
        assert np.abs(ref['bures2'][at] - row[6]).max() <= 2.0 ** -26 * 20
        assert np.abs(ref['jeffreys'][at] - row[7]).max() <= 1e-13 * (abs(row[7]) + 6) + (2e-7 if row[7] > 1e6 else 0)  # 6499998.0000002: 14 digits


# ---------------------------------------------------------------- the host build
@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no C++ compiler')
    src = os.path.join(os.path.dirname(__file__), 'csrc', 'compare_check.cpp')
    out = str(tmp_path_factory.mktemp('compare_check') / 'compare_check')
    flags = ['-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']
    if subprocess.run([cxx, *flags, '-o', out, src], capture_output=True).returncode != 0:   # (no sanitizer runtime installed)
        subprocess.run([cxx, '-O1', '-std=c++17', '-o', out, src], check=True)
    return out


def host_eval(exe, tmp_path, states, n_a, n_b, scale, std_floor=P.STD_FLOOR):
    """compare_maps of the host build on float32 states -> (planes dict, tr_a, tr_b, finite, floored), shaped like the states"""
    ma, Ma, mb, Mb = (np.ascontiguousarray(x, dtype=np.float32) for x in states)
    shape = ma.shape[1:]
    V = int(np.prod(shape))
    src, dst = str(tmp_path / 'states.bin'), str(tmp_path / 'planes.bin')
    with open(src, 'wb') as f:
        np.array([V, n_a, n_b], dtype=np.int64).tofile(f)
        np.array([*scale, std_floor], dtype=np.float64).tofile(f)
        for x in (ma, Ma, mb, Mb):
            x.tofile(f)
    out = subprocess.run([exe, 'eval', src, dst], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = open(dst, 'rb').read()
    planes = np.frombuffer(raw, dtype=np.float32, count=4 * V).reshape((4,) + shape)
    tr = np.frombuffer(raw, dtype=np.float64, count=2 * V, offset=16 * V).reshape((2,) + shape)
    flags = np.frombuffer(raw, dtype=np.uint8, count=2 * V, offset=32 * V).reshape((2,) + shape).astype(bool)
    return dict(zip(P.PLANES, planes)), tr[0], tr[1], flags[0], flags[1]


def test_closed_forms_and_invariants_of_the_host_build(exe):
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'violations 0' in out.stdout
    worst = {name: float(v) for name, v in re.findall(r'^worst ([a-z_, ]+?) ([0-9.eE+\-]+|inf|nan)$', out.stdout, flags=re.M)}
    assert set(worst) == {'known', 'log_std_ratio', 'bures', 'jeffreys', 'jeffreys, rounded inputs'}
    # an invariant sets two evaluations against one another: twice the constant of one against the restatement
    assert worst['known'] <= 1.0 and worst['log_std_ratio'] <= 1.0
    assert worst['bures'] <= 2 * P.C_B, worst
    assert worst['jeffreys'] <= 2 * P.C_J and worst['jeffreys, rounded inputs'] <= 2 * P.C_J, worst


def all_cases():
    """(label, states, n_a, n_b, scale) of every case the GPU test compares with the restatement, states in float32 numpy"""
    ma, Ma, mb, Mb, _ = P.known_states()
    yield 'known', (ma, Ma, mb, Mb), *P.KNOWN_N, (1.0, 1.0, 1.0)
    for recipe in P.RECIPES:
        for shape in P.SHAPES:
            for n_a, n_b in P.RECORDS:
                a, b = P.draw_pair(recipe, shape, n_a, n_b)
                yield f'{recipe} {shape} {n_a} vs {n_b}', P.host_states(a, b), n_a, n_b, P.default_scale(shape)
                st = P.host_states(a, a)
                yield f'{recipe} {shape} {n_a} identical', st, n_a, n_a, P.default_scale(shape)
        a, b = P.draw_pair(recipe, P.SHAPES[0], *P.RECORDS[0])
        yield f'{recipe} own scale', P.host_states(a, b), *P.RECORDS[0], P.OWN_SCALE


def test_host_build_matches_the_restatement(exe, tmp_path):
    """the measurement behind C_B and C_J, and the check that the host build stays inside the tolerances they give"""
    worst = {'bures': 0.0, 'jeffreys': 0.0}
    for label, states, n_a, n_b, scale in all_cases():
        ref = P.compare_np(states[0], states[1], n_a, states[2], states[3], n_b, scale)
        planes, tr_a, tr_b, finite, floored = host_eval(exe, tmp_path, states, n_a, n_b, scale)
        r = P.ratios(ref, planes)
        print(label, r)
        for k in worst:
            worst[k] = max(worst[k], r[k][1])
        assert finite.all() and np.array_equal(floored, ref['floored']), label
        assert np.allclose(tr_a, ref['tr_a'], rtol=1e-14, atol=0) and np.allclose(tr_b, ref['tr_b'], rtol=1e-14, atol=0)
        P.check_planes(ref, planes, label)
        if 'identical' in label:
            assert not planes['shift'].any() and not planes['log_std_ratio'].any()
    print('worst ratios in units of the bound forms with c = 1:', worst)
    assert worst['bures'] <= P.C_B and worst['jeffreys'] <= P.C_J, worst


def test_non_finite_states_give_nan_in_the_host_build(exe, tmp_path):
    a, b = P.draw_pair('anisotropic', (5, 7, 9), 4, 6)
    ma, Ma, mb, Mb = (x.copy() for x in P.host_states(a, b))
    ma[1, 0, 0, 0], Mb[4, 1, 2, 3], Ma[0, 4, 6, 8] = np.nan, np.inf, -np.inf
    ref = P.compare_np(ma, Ma, 4, mb, Mb, 6, (1.0, 1.0, 1.0))
    planes, _, _, finite, _ = host_eval(exe, tmp_path, (ma, Ma, mb, Mb), 4, 6, (1.0, 1.0, 1.0))
    assert (~finite).sum() == 3 and np.array_equal(finite, ref['finite'])
    P.check_planes(ref, planes)


# ---------------------------------------------------------------- the option
BASE = {'VI': True, 'MCMC': True, 'no_samples_VI_test': 4, 'no_samples_MCMC': 8, 'no_chains': 2, 'log_period_MCMC': 4}


def test_option_parsing():
    opt = posterior_comparison_options
    assert opt(BASE) is None and opt({**BASE, 'posterior_comparison': False}) is None
    assert opt({**BASE, 'posterior_comparison': None}) is None
    assert opt({**BASE, 'posterior_comparison': True}) == {'period': 4, 'std_floor': 1e-3}
    assert opt({**BASE, 'posterior_comparison': {'period': 2}}) == {'period': 2, 'std_floor': 1e-3}
    assert opt({**BASE, 'posterior_comparison': {'std_floor': 0.5}}) == {'period': 4, 'std_floor': 0.5}
    assert opt({**BASE, 'VI': False, 'resume': 'x.pt', 'posterior_comparison': True}) == {'period': 4, 'std_floor': 1e-3}
    for over, message in (
            ({'posterior_comparison': {'periods': 2}}, r"unknown keys \['periods'\]"),
            ({'posterior_comparison': 3}, 'must be true, false or'),
            ({'posterior_comparison': {'period': 2.0}}, 'period must be an integer'),
            ({'posterior_comparison': {'period': 0}}, 'the period must be >= 1'),
            ({'posterior_comparison': {'period': 16}}, 'records no step'),
            ({'posterior_comparison': {'std_floor': 0}}, 'std_floor must be a finite number > 0, got 0'),
            ({'posterior_comparison': {'std_floor': -1e-3}}, 'std_floor must be a finite number > 0'),
            ({'posterior_comparison': {'std_floor': float('nan')}}, 'std_floor must be a finite number > 0'),
            ({'posterior_comparison': {'std_floor': float('inf')}}, 'std_floor must be a finite number > 0'),
            ({'posterior_comparison': {'std_floor': '1e-3'}}, 'std_floor must be a finite number > 0'),
            ({'posterior_comparison': {'std_floor': True}}, 'std_floor must be a finite number > 0'),
            ({'posterior_comparison': True, 'MCMC': False}, 'needs the MCMC stage'),
            ({'posterior_comparison': True, 'VI': False}, 'needs the VI stage'),
            ({'posterior_comparison': True, 'no_samples_VI_test': 3}, r'no_samples_VI_test = 3.*at least 4'),
            ({'posterior_comparison': {'period': 8}, 'no_chains': 2}, r'no_samples_MCMC = 8 with period 8.*2 records.*at least 4'),
            ({'posterior_comparison': {'period': 4}, 'no_chains': 1}, r'1 steps of 1 chains|2 steps of 1 chains')):
        with pytest.raises(ValueError, match=message):
            opt({**BASE, **over})
    # exactly four records on either side are enough
    assert opt({**BASE, 'posterior_comparison': {'period': 4}}) is not None  # 2 steps x 2 chains


def test_init_metrics_names_the_comparison_last_and_only_when_on(tmp_path):
    import copy
    import json
    from ir_sgmcmc_amd.parse_config import ConfigParser
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = json.load(open(os.path.join(root, 'configs', 'synthetic_gmm_lognormal.json')))
    cfg['trainer']['save_dir'] = str(tmp_path)
    cfg['trainer'].update(VI=True, no_samples_VI_test=4, no_samples_MCMC=8, no_chains=2, log_period_MCMC=2, residual_check=True)
    off = ConfigParser.from_dict(copy.deepcopy(cfg), timestamp='t').init_metrics()
    cfg['trainer']['posterior_comparison'] = {'period': 2}
    on = ConfigParser.from_dict(copy.deepcopy(cfg), timestamp='t').init_metrics()
    names = [f'MCMC/vs_VI/{k}' for k in COMPARISON_METRICS]
    assert on == off + names and not [m for m in off if 'vs_VI' in m]
    assert COMPARISON_METRICS == P.FLOAT_KEYS


# ---------------------------------------------------------------- the summary
def test_comparison_summary_on_hand_made_columns():
    isum = [10, 2, 3, 6]
    fsum = [16.0, 5.0, -4.0, -2.0, 1.0, 8.0, 3.0, 24.0, 6.0, 40.0, 30.0, 72.0, 32.0]
    s = comparison_summary(isum, fsum, 4, 16)
    assert list(s) == list(P.INT_KEYS) + list(P.FLOAT_KEYS)
    assert (s['records_vi'], s['records_mcmc'], s['voxels'], s['nonfinite_voxels'], s['floored_voxels']) == (4, 16, 10, 2, 3)
    want = {'shift_mean': 2.0, 'shift_max': 5.0, 'log_std_ratio_mean': -0.5, 'log_std_ratio_min': -2.0, 'log_std_ratio_max': 1.0,
            'std_ratio': math.exp(-0.5), 'frac_vi_narrower': 0.75, 'bures_mean': 1.0, 'bures_max': 3.0, 'w2_mean': 3.0, 'w2_max': 6.0,
            'jeffreys_mean': 5.0, 'jeffreys_max': 30.0, 'std_total_vi': 3.0, 'std_total_mcmc': 2.0}
    for k, v in want.items():
        assert s[k] == pytest.approx(v, rel=1e-15), k
    inf = float('inf')
    for isum in ([0, 0, 0, 0], [5, 5, 0, 0]):  # an empty mask; no masked voxel finite
        e = comparison_summary(isum, [0.0, -inf, 0.0, inf, -inf, 0.0, -inf, 0.0, -inf, 0.0, -inf, 0.0, 0.0], 4, 16)
        assert e['voxels'] == isum[0] and e['nonfinite_voxels'] == isum[1] and all(math.isnan(e[k]) for k in P.FLOAT_KEYS)
