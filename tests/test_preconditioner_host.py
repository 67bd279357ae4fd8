"""The adaptive preconditioner without a GPU: exact dyadic cases of the numpy restatement (tests/_preconditioner.py), worked out by
hand in the manner of tests/_exact_cases.py, every refusal of the option, and the checkpoint key rules."""
import numpy as np
import pytest
import torch

from ir_sgmcmc_amd import preconditioner as P
from tests import _preconditioner as S

f32 = np.float32
DIMS = (3, 4, 5)


def signs(shape, seed):
    return np.where(np.random.default_rng(seed).random(shape) < 0.5, -1.0, 1.0).astype(f32)


# ---------------------------------------------------------------- exact cases
@pytest.mark.parametrize('C', [1, 2, 3])
@pytest.mark.parametrize('k', [-3, 0, 5])
def test_constant_magnitude_gives_the_closed_form_and_a_flat_sigma(C, k):
    """|g| = 2^k everywhere and beta = 1/2: V_t = g^2 (1 - 2^-t), every step exact (C g^2 / C is an exact quotient).  The
    corrected field is uniform, so every mean is one of its own terms and sigma is 1 in every bit, smoothed or not."""
    V = np.zeros((1, 3, *DIMS), f32)
    for t in range(1, 8):
        g = signs((C, 3, *DIMS), 10 * t + C) * f32(2.0 ** k)
        V, bad = S.accumulate(V, g, None, 0.5)
        assert bad == 0
        assert (V == f32(4.0 ** k * (1.0 - 2.0 ** -t))).all()
        for r in (0, 1, 2):
            sigma, summary = S.sigma_field(V, C, S.bias_correction(0.5, t), r, 0.1, 0.25, 4.0)
            assert sigma.shape == (C, 3, *DIMS) and (sigma == f32(1.0)).all()
            assert summary['sigma_min'] == summary['sigma_max'] == summary['sigma2_mean'] == 1.0
            assert summary['clamped_low'] == summary['clamped_high'] == 0
            assert summary['s_mean'] == float(np.sqrt(S.corrected(V, S.bias_correction(0.5, t), r))[0, 0, 0, 0])


def test_sigma_of_ones_has_the_bits_of_no_sigma():
    rng = np.random.default_rng(0)
    V = rng.random((1, 3, *DIMS)).astype(f32)
    g = rng.standard_normal((2, 3, *DIMS)).astype(f32)
    a, _ = S.accumulate(V, g, None, 0.9)
    b, _ = S.accumulate(V, g, np.ones_like(g), 0.9)
    assert a.tobytes() == b.tobytes()
    # a sigma of 2 everywhere: g = grad_v / 4 exactly, so V moves by a sixteenth of the increment
    c, _ = S.accumulate(np.zeros_like(V), g, np.full_like(g, 2.0), 0.5)
    d, _ = S.accumulate(np.zeros_like(V), g, None, 0.5)
    assert (c == d / f32(16.0)).all()


def test_no_gradient_gives_sigma_one():
    V = np.zeros((1, 3, *DIMS), f32)
    V, bad = S.accumulate(V, np.zeros((2, 3, *DIMS), f32), None, 0.99)
    assert bad == 0 and not V.any()
    for count in (0, 1):
        sigma, summary = S.sigma_field(V, 2, S.bias_correction(0.99, count), 1, 0.1, 0.25, 4.0)
        assert (sigma == f32(1.0)).all() and summary['s_mean'] == 0.0 and summary['G_mean'] == 1.0
        assert summary['clamped_low'] == summary['clamped_high'] == 0


@pytest.mark.parametrize('r', [0, 1, 2])
@pytest.mark.parametrize('j', [-4, 3])
def test_scaling_the_gradient_by_a_power_of_four_leaves_sigma_bit_identical(r, j):
    rng = np.random.default_rng(5)
    V0, V1 = np.zeros((1, 3, *DIMS), f32), np.zeros((1, 3, *DIMS), f32)
    for t in range(1, 4):
        g = (rng.standard_normal((2, 3, *DIMS)) + 0.1).astype(f32)
        V0, _ = S.accumulate(V0, g, None, 0.75)
        V1, _ = S.accumulate(V1, g * f32(4.0 ** j), None, 0.75)
    assert (V1 == V0 * f32(16.0 ** j)).all()
    bias = S.bias_correction(0.75, 3)
    a, sa = S.sigma_field(V0, 1, bias, r, 0.1, 0.25, 4.0)
    b, sb = S.sigma_field(V1, 1, bias, r, 0.1, 0.25, 4.0)
    assert a.tobytes() == b.tobytes()
    assert sb['s_mean'] == sa['s_mean'] * 4.0 ** j and sb['G_mean'] == sa['G_mean'] * 4.0 ** -j
    assert float(a.min()) < 1.0 < float(a.max())  # the field is not flat: the case says something


def test_a_two_level_field_hits_both_clamps():
    """N = 72 elements: 48 with V = 1 (s = 1) and 24 with V = 2^20 (s = 1024), bias 1, no smoothing, damping 2^-10.
    sbar = (48 + 24 * 1024) / 72 = 342, lambda = 342 / 1024 = 0.333984375 (exact).  G = 1 / 1.333984375 = 0.74964 and
    1 / 1024.333984375 = 0.00097624; Gbar = (48 * 0.74964 + 24 * 0.00097624) / 72 = 0.50008.  raw = sqrt(G / Gbar) = 1.2243 and
    0.044183: with the clamp [0.25, 1.125] all 48 are clamped high and all 24 low, and the mean of sigma^2 is
    (48 * 1.265625 + 24 * 0.0625) / 72 = 62.25 / 72."""
    V = np.ones((1, 3, 2, 3, 4), f32)
    V.reshape(-1)[48:] = f32(2.0 ** 20)
    sigma, summary = S.sigma_field(V, 3, 1.0, 0, 2.0 ** -10, 0.25, 1.125, nonfinite=7)
    flat = sigma.reshape(3, -1)
    assert (flat[:, :48] == f32(1.125)).all() and (flat[:, 48:] == f32(0.25)).all()
    assert summary['s_mean'] == 342.0
    assert summary['G_mean'] == pytest.approx((48 / 1.333984375 + 24 / 1024.333984375) / 72, rel=1e-6)
    assert (summary['clamped_low'], summary['clamped_high']) == (24, 48)
    assert (summary['sigma_min'], summary['sigma_max'], summary['sigma2_mean']) == (0.25, 1.125, 62.25 / 72)
    assert summary['nonfinite'] == 7


def test_box_mean_of_a_single_spike():
    """one voxel of 27 in a zero channel, r = 1, away from the border: the 27 voxels around it hold 1, everything else 0; in a
    corner the replicate padding counts the corner voxel 8 times: 8 * 27 / 27 = 8 there"""
    V = np.zeros((1, 3, 5, 6, 7), f32)
    V[0, 0, 2, 3, 3] = 27.0
    V[0, 1, 0, 0, 0] = 27.0
    out = S.corrected(V, 1.0, 1)
    want = np.zeros((5, 6, 7), f32)
    want[1:4, 2:5, 2:5] = 1.0
    assert (out[0] == want).all()
    assert out[1, 0, 0, 0] == 8.0 and out[1, 1, 1, 1] == 1.0 and out[1, 0, 0, 1] == 4.0 and out[1, 2, 0, 0] == 0.0
    assert not out[2].any()


def test_a_non_finite_gradient_is_counted():
    g = np.ones((2, 3, *DIMS), f32)
    g[1, 2, 0, 0, 0], g[0, 0, 1, 1, 1] = np.nan, np.inf
    _, bad = S.accumulate(np.zeros((1, 3, *DIMS), f32), g, None, 0.5)
    assert bad == 2


# ---------------------------------------------------------------- the option
BASE = {'MCMC_init': 'identity'}
WHAT = 'trainer.adaptive_preconditioner'


def test_option_absent_is_none():
    assert P.adaptive_preconditioner_options({}, 50) is None
    assert P.adaptive_preconditioner_options({'MCMC_init': 'VI'}, 0) is None
    assert P.adaptive_preconditioner_options({'adaptive_preconditioner': None}, 50) is None


def test_option_defaults_and_values():
    assert P.adaptive_preconditioner_options({**BASE, 'adaptive_preconditioner': {}}, 120) == {
        'beta': 0.99, 'refresh': 50, 'until': 120, 'damping': 0.1, 'smooth': 1, 'sigma_min': 0.25, 'sigma_max': 4.0, 'save': True}
    opt = {'beta': 0, 'refresh': 4, 'until': 8, 'damping': 2, 'smooth': 0, 'sigma_min': 1, 'sigma_max': 1, 'save': False}
    got = P.adaptive_preconditioner_options({'MCMC_init': 'coarse', 'adaptive_preconditioner': opt}, 12)
    assert got == {'beta': 0.0, 'refresh': 4, 'until': 8, 'damping': 2.0, 'smooth': 0, 'sigma_min': 1.0, 'sigma_max': 1.0, 'save': False}
    assert [P.is_refresh(t, got) for t in range(1, 11)] == [False, False, False, True, False, False, False, True, False, False]
    odd = {**got, 'refresh': 3, 'until': 7}
    assert [t for t in range(1, 12) if P.is_refresh(t, odd)] == [3, 6, 7]


REFUSALS = [
    ([1, 2], 12, f'{WHAT} must be a dict with the optional keys'),
    ({'decay': 0.9}, 12, f"{WHAT}: unknown keys ['decay']; known: "),
    ({'beta': '0.9'}, 12, f"{WHAT}.beta must be a number, got '0.9'"),
    ({'beta': True}, 12, f'{WHAT}.beta must be a number, got True'),
    ({'beta': 1.0}, 12, f'{WHAT}.beta must be in [0, 1), got 1.0'),
    ({'beta': -0.1}, 12, f'{WHAT}.beta must be in [0, 1), got -0.1'),
    ({'beta': float('nan')}, 12, f'{WHAT}.beta must be in [0, 1), got nan'),
    ({'refresh': 0}, 12, f'{WHAT}.refresh must be >= 1, got 0'),
    ({'refresh': 2.0}, 12, f'{WHAT}.refresh must be an integer, got 2.0'),
    ({'refresh': False}, 12, f'{WHAT}.refresh must be an integer, got False'),
    ({'until': 13}, 12, f'{WHAT}.until must be in 1 .. no_iters_burn_in = 12 (the recorded chain must run on a frozen sigma), got 13'),
    ({'until': 0}, 12, f'{WHAT}.until must be in 1 .. no_iters_burn_in = 12 (the recorded chain must run on a frozen sigma), got 0'),
    ({'until': 1.5}, 12, f'{WHAT}.until must be an integer, got 1.5'),
    ({'damping': 0}, 12, f'{WHAT}.damping must be a finite number > 0, got 0.0'),
    ({'damping': float('inf')}, 12, f'{WHAT}.damping must be a finite number > 0, got inf'),
    ({'damping': None}, 12, f'{WHAT}.damping must be a number, got None'),
    ({'smooth': 3}, 12, f'{WHAT}.smooth must be in 0 .. 2, got 3'),
    ({'smooth': -1}, 12, f'{WHAT}.smooth must be in 0 .. 2, got -1'),
    ({'smooth': True}, 12, f'{WHAT}.smooth must be an integer, got True'),
    ({'sigma_min': 0}, 12, f'{WHAT}: 0 < sigma_min <= 1 <= sigma_max < inf needed, got sigma_min = 0.0, sigma_max = 4.0'),
    ({'sigma_min': 1.5}, 12, f'{WHAT}: 0 < sigma_min <= 1 <= sigma_max < inf needed, got sigma_min = 1.5, sigma_max = 4.0'),
    ({'sigma_max': 0.5}, 12, f'{WHAT}: 0 < sigma_min <= 1 <= sigma_max < inf needed, got sigma_min = 0.25, sigma_max = 0.5'),
    ({'sigma_max': float('inf')}, 12, f'{WHAT}: 0 < sigma_min <= 1 <= sigma_max < inf needed, got sigma_min = 0.25, sigma_max = inf'),
    ({'sigma_max': [4]}, 12, f'{WHAT}.sigma_max must be a number, got [4]'),
    ({'save': 1}, 12, f'{WHAT}.save must be true or false, got 1'),
    ({}, 0, f'{WHAT}: no_iters_burn_in = 0; the preconditioner is adapted during burn-in only'),
]


@pytest.mark.parametrize('opt,burn_in,message', REFUSALS)
def test_option_refusals(opt, burn_in, message):
    with pytest.raises(ValueError) as e:
        P.adaptive_preconditioner_options({**BASE, 'adaptive_preconditioner': opt}, burn_in)
    assert str(e.value).startswith(message), str(e.value)


def test_option_refuses_a_vi_start():
    with pytest.raises(ValueError) as e:
        P.adaptive_preconditioner_options({'MCMC_init': 'VI', 'adaptive_preconditioner': {}}, 12)
    assert str(e.value) == f'{WHAT}: trainer.MCMC_init = "VI" is not supported (sigma is the VI posterior\'s standard deviation there)'


# ---------------------------------------------------------------- the checkpoint key
def test_checkpoint_key_rules():
    opt = P.adaptive_preconditioner_options({**BASE, 'adaptive_preconditioner': {'until': 8}}, 12)
    state = {'V': torch.arange(3 * 8, dtype=torch.float32).reshape(1, 3, 2, 2, 2), 'count': 6, 'nonfinite': torch.tensor([3])}
    entry = P.checkpoint_entry(state, None)
    assert set(entry) == {'V', 'count', 'nonfinite', 'frozen'} and entry['count'] == 6 and entry['nonfinite'] == 3
    assert entry['frozen'] == -1 and torch.equal(entry['V'], state['V'])
    assert P.checkpoint_entry(state, 8)['frozen'] == 8
    # the option off: never a complaint; on: a checkpoint without the key is refused up to `until`, accepted past it
    P.check_checkpoint({}, None, 3)
    P.check_checkpoint({'preconditioner': entry}, opt, 3)
    P.check_checkpoint({}, opt, 9)
    for sample_no in (1, 8):
        with pytest.raises(ValueError) as e:
            P.check_checkpoint({}, opt, sample_no)
        assert str(e.value) == (f'the checkpoint at sample {sample_no} holds no preconditioner state (written with '
                                f'trainer.adaptive_preconditioner off) but this run adapts sigma until transition 8')


def test_bias_correction():
    assert P.bias_correction(0.5, 0) == 1.0 and P.bias_correction(0.5, 1) == 2.0 and P.bias_correction(0.5, 3) == 1.0 / 0.875
    assert P.bias_correction(0.0, 4) == 1.0
    assert P.bias_correction(0.99, 7) == S.bias_correction(0.99, 7)
