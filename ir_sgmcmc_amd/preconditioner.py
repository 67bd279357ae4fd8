"""Adaptive pSGLD: the diagonal RMSprop preconditioner of Li et al. 2016, estimated during burn-in and then frozen, and the
`trainer.adaptive_preconditioner` option.

The sigma field of a chain is otherwise the VI posterior's standard deviation (`MCMC_init: "VI"`) or 1.  Here a second moment V of
the gradient dL/dv_s, shared by the chains, is updated after every adapting transition (`preconditioner_accumulate`:
irs_precond_accumulate) and turned into a sigma field at every refresh (`preconditioner_sigma`: irs_precond_sigma): bias
correction, an optional box mean, G = 1 / (damping * mean(sqrt V) + sqrt V), sigma = clamp(sqrt(G / mean G)).  The field is
normalised so that the mean of G / mean G is 1: the learning rate keeps its meaning.  Adaptation stops at `until`, within the
burn-in: the recorded samples then come from an SGLD with a fixed sigma field, as after a VI stage.  While sigma changes, pSGLD
needs its correction term Gamma, which is not implemented -- hence the limit.  include/irsgmcmc.h has the arithmetic, element by
element.

The operator wrappers live here and not in ops.py; they use its private helpers.
"""
import ctypes
import numbers

import torch

from . import _lib as L
from .ops import _call, _workspace

OPTION_KEYS = ('beta', 'refresh', 'until', 'damping', 'smooth', 'sigma_min', 'sigma_max', 'save')
SUMMARY_KEYS = ('s_mean', 'G_mean', 'sigma_min', 'sigma_max', 'sigma2_mean', 'clamped_low', 'clamped_high', 'nonfinite')
METRICS = ('sigma_min', 'sigma_max', 'sigma2_mean', 'clamped_low', 'clamped_high')


def preconditioner_state(v_shape, device):
    """v_shape: the velocity grid (Dv, Hv, Wv), or any shape that ends in it -> {'V': (1,3,Dv,Hv,Wv) float32 zeros, the second
    moment shared by the chains; 'count': updates so far; 'nonfinite': one int64 on the device, the non-finite gradients seen}"""
    dims = tuple(int(n) for n in tuple(v_shape)[-3:])
    if len(dims) != 3 or min(dims) < 1:
        raise L.IrsError(f'v_shape must end in the velocity grid (Dv, Hv, Wv), got {tuple(v_shape)!r}')
    return {'V': torch.zeros((1, 3, *dims), device=device, dtype=torch.float32), 'count': 0,
            'nonfinite': torch.zeros(1, device=device, dtype=torch.int64)}


def _state(state):
    V = state['V']
    if V.dim() != 5 or V.shape[:2] != (1, 3):
        raise L.IrsError(f'state["V"] must have shape (1,3,Dv,Hv,Wv), got {tuple(V.shape)}')
    return V, tuple(V.shape[2:])


def preconditioner_accumulate(grad_v, sigma, state, beta):
    """One update of the second moment with the gradients of all chains: grad_v (C,3,Dv,Hv,Wv) float32 as a transition hands it
    out (sigma^2 dL/dv_s), sigma (C,3,Dv,Hv,Wv) the field that transition ran with, or None (= 1).  V <- beta V + (1 - beta) mean
    over the chains of (grad_v / sigma^2)^2; state['count'] += 1.  One launch; no host synchronisation."""
    V, dims = _state(state)
    if grad_v.dim() != 5 or tuple(grad_v.shape[1:]) != (3, *dims):
        raise L.IrsError(f'grad_v must have shape (C,3,{dims[0]},{dims[1]},{dims[2]}), got {tuple(grad_v.shape)}')
    if sigma is not None and sigma.shape != grad_v.shape:
        raise L.IrsError(f'sigma must have the shape of grad_v {tuple(grad_v.shape)}, got {tuple(sigma.shape)}')
    _call('irs_precond_accumulate', L.dev_ptr(grad_v, torch.float32), L.dev_ptr(sigma, torch.float32, allow_none=True),
          grad_v.shape[0], *dims, float(beta), L.dev_ptr(V, torch.float32), L.dev_ptr(state['nonfinite'], torch.int64))
    state['count'] += 1


def bias_correction(beta, count):
    """1 / (1 - beta^count) in double; 1 before the first update (V is zero then, and so is every corrected value)"""
    return 1.0 if count < 1 else 1.0 / (1.0 - float(beta) ** int(count))


def preconditioner_sigma(state, C, beta, smooth=1, damping=0.1, sigma_min=0.25, sigma_max=4.0):
    """The sigma field of the second moment as it stands -> (sigma (C,3,Dv,Hv,Wv) float32, the same field for every chain,
    summary dict of SUMMARY_KEYS).  `beta` must be the one the state was accumulated with (it enters the bias correction only).
    Blocking: the summary is read back."""
    V, dims = _state(state)
    if isinstance(C, bool) or not isinstance(C, numbers.Integral):
        raise L.IrsError(f'C must be an integer, got {C!r}')
    if isinstance(smooth, bool) or not isinstance(smooth, numbers.Integral):
        raise L.IrsError(f'smooth must be an integer, got {smooth!r}')
    if not 0.0 <= float(beta) < 1.0:
        raise L.IrsError(f'beta = {beta!r}, a value in [0, 1) needed')
    ws, ws_bytes = _workspace('irs_precond_workspace', *dims, int(smooth), device=V.device)
    sigma = torch.empty((max(int(C), 0), 3, *dims), device=V.device, dtype=torch.float32)
    summary = torch.empty(L.IRS_PRECOND_SUMMARY, device=V.device, dtype=torch.float64)
    _call('irs_precond_sigma', L.dev_ptr(V, torch.float32), int(C), *dims, ctypes.c_double(bias_correction(beta, state['count'])),
          int(smooth), ctypes.c_double(float(damping)), float(sigma_min), float(sigma_max), L.dev_ptr(state['nonfinite'], torch.int64),
          L.dev_ptr(sigma), L.dev_ptr(summary), L.dev_ptr(ws), ws_bytes)
    row = summary.tolist()
    out = dict(zip(SUMMARY_KEYS, row))
    for key in ('clamped_low', 'clamped_high', 'nonfinite'):
        out[key] = int(out[key])
    return sigma, out


def _number(what, key, value, integer=False):
    kind = numbers.Integral if integer else numbers.Real
    if isinstance(value, bool) or not isinstance(value, kind):
        raise ValueError(f'{what}.{key} must be {"an integer" if integer else "a number"}, got {value!r}')
    return int(value) if integer else float(value)


def adaptive_preconditioner_options(cfg_trainer, no_iters_burn_in):
    """`trainer.adaptive_preconditioner = {"beta": 0.99, "refresh": 50, "until": <no_iters_burn_in>, "damping": 0.1, "smooth": 1,
    "sigma_min": 0.25, "sigma_max": 4.0, "save": true}`, every key optional -> None when the option is absent (and then nothing
    anywhere changes), else the dict with every key filled in.

    beta: the decay of the second moment.  refresh: sigma is recomputed every `refresh` transitions, and at `until`.  until: the
    last adapting transition; afterwards sigma is frozen.  damping: lambda = damping * mean(sqrt V) is added to sqrt V, which
    bounds the ratio of the largest to the smallest step.  smooth: half-width r of the (2r+1)^3 box mean of V (0: none).
    sigma_min / sigma_max: the clamp.  save: on SVF_3D, write the per-voxel RMS of sigma over the three channels at the freeze.
    The defaults are choices for the user to tune, NOT measured optima.

    Refuses unknown keys, wrong types (booleans as numbers too), beta outside [0, 1), refresh < 1, until < 1 or > no_iters_burn_in
    (the recorded chain must run on a frozen sigma), damping <= 0, smooth outside 0 .. 2, sigma_min / sigma_max outside 0 <
    sigma_min <= 1 <= sigma_max < inf, a burn-in of 0, and MCMC_init "VI" (sigma is the VI posterior's there)."""
    what = 'trainer.adaptive_preconditioner'
    opt = cfg_trainer.get('adaptive_preconditioner')
    if opt is None:
        return None
    if not isinstance(opt, dict):
        raise ValueError(f'{what} must be a dict with the optional keys {list(OPTION_KEYS)}, got {opt!r}')
    unknown = set(opt) - set(OPTION_KEYS)
    if unknown:
        raise ValueError(f'{what}: unknown keys {sorted(unknown)}; known: {list(OPTION_KEYS)}')
    if cfg_trainer.get('MCMC_init') == 'VI':
        raise ValueError(f'{what}: trainer.MCMC_init = "VI" is not supported (sigma is the VI posterior\'s standard deviation there)')
    burn_in = int(no_iters_burn_in)
    if burn_in < 1:
        raise ValueError(f'{what}: no_iters_burn_in = {burn_in}; the preconditioner is adapted during burn-in only, so a burn-in '
                         f'of at least 1 transition is needed')
    beta = _number(what, 'beta', opt.get('beta', 0.99))
    if not 0.0 <= beta < 1.0:
        raise ValueError(f'{what}.beta must be in [0, 1), got {beta!r}')
    refresh = _number(what, 'refresh', opt.get('refresh', 50), integer=True)
    if refresh < 1:
        raise ValueError(f'{what}.refresh must be >= 1, got {refresh}')
    until = _number(what, 'until', opt.get('until', burn_in), integer=True)
    if until < 1 or until > burn_in:
        raise ValueError(f'{what}.until must be in 1 .. no_iters_burn_in = {burn_in} (the recorded chain must run on a frozen '
                         f'sigma), got {until}')
    damping = _number(what, 'damping', opt.get('damping', 0.1))
    if not damping > 0.0 or damping == float('inf'):
        raise ValueError(f'{what}.damping must be a finite number > 0, got {damping!r}')
    smooth = _number(what, 'smooth', opt.get('smooth', 1), integer=True)
    if not 0 <= smooth <= L.IRS_PRECOND_MAX_SMOOTH:
        raise ValueError(f'{what}.smooth must be in 0 .. {L.IRS_PRECOND_MAX_SMOOTH}, got {smooth}')
    sigma_min = _number(what, 'sigma_min', opt.get('sigma_min', 0.25))
    sigma_max = _number(what, 'sigma_max', opt.get('sigma_max', 4.0))
    if not (0.0 < sigma_min <= 1.0 <= sigma_max < float('inf')):
        raise ValueError(f'{what}: 0 < sigma_min <= 1 <= sigma_max < inf needed, got sigma_min = {sigma_min!r}, sigma_max = '
                         f'{sigma_max!r}')
    save = opt.get('save', True)
    if not isinstance(save, bool):
        raise ValueError(f'{what}.save must be true or false, got {save!r}')
    return {'beta': beta, 'refresh': refresh, 'until': until, 'damping': damping, 'smooth': smooth, 'sigma_min': sigma_min,
            'sigma_max': sigma_max, 'save': save}


def is_refresh(step, options):
    """whether sigma is recomputed after adapting transition `step` (1-based)"""
    return step <= options['until'] and (step % options['refresh'] == 0 or step == options['until'])


def checkpoint_entry(state, frozen_at):
    """what a checkpoint keeps of the estimator: plain tensors and numbers"""
    return {'V': state['V'].detach().cpu(), 'count': int(state['count']), 'nonfinite': int(state['nonfinite'].item()),
            'frozen': -1 if frozen_at is None else int(frozen_at)}


def check_checkpoint(sd, options, sample_no):
    """The checkpoint key rules: with the option on, a checkpoint taken at sample_no <= until must hold 'preconditioner' (its V
    is needed to go on adapting); past `until` sigma is frozen and the checkpoint's own 'sigma' is all a resumed run needs."""
    if options is None or 'preconditioner' in sd or sample_no > options['until']:
        return
    raise ValueError(f'the checkpoint at sample {sample_no} holds no preconditioner state (written with '
                     f'trainer.adaptive_preconditioner off) but this run adapts sigma until transition {options["until"]}')
