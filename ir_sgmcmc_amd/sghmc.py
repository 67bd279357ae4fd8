"""SGHMC: stochastic-gradient Hamiltonian Monte Carlo (Chen, Fox & Guestrin 2014, eq. 15 with beta_hat = 0) as a second sampler
next to the reference's scheme, and the `trainer.sampler` option.

The reference's transition draws fresh noise in front of the forward pass, records the smoothed noisy field and lets v itself do
noisy gradient descent: nothing of the noise stays in v.  With `"type": "SGHMC"` the forward pass adds none; per element of the
velocity grid the update is, in float32 with every operation rounded once (csrc/sghmc_device.h),

    t  = (1 - friction) m - lr grad_v
    m' = t + sqrt(2 friction lr T) sigma n        (T > 0; n a standard normal, Philox stream word 0x484D)
    v' = v + m'

friction = 1 is Langevin dynamics whose noise is persisted in v, friction < 1 adds momentum, T = 0 draws no noise at all (a
heavy-ball MAP optimiser).  With `Sobolev_grad` on, grad_v is not the gradient of a potential in v -- the smoothing's backward is
the identity, as in the reference -- so the chain is the persistent-noise, momentum counterpart of the reference's heuristic; it is
textbook SGHMC only with the smoothing off.

The operator wrapper lives here and not in ops.py; it uses its private helper.
"""
import numbers

import torch

from . import _lib as L
from .ops import _call

SAMPLERS = ('SGLD', 'SGHMC')
OPTION_KEYS = ('type', 'friction', 'temperature')
DEFAULT_FRICTION = 0.1      # a choice for the user to tune, NOT a measured optimum
DEFAULT_TEMPERATURE = 1.0


def _check_numbers(what, friction, temperature):
    if not 0.0 < friction <= 1.0:
        raise ValueError(f'{what}friction must be in (0, 1], got {friction!r}')
    if not 0.0 <= temperature < float('inf'):
        raise ValueError(f'{what}temperature must be a finite number >= 0, got {temperature!r}')


def sghmc_update(v, momentum, grad, sigma=None, *, lr, friction, temperature=1.0, seed=0, iteration=0, eps=None):
    """irs_sghmc_update: one SGHMC step on (v, momentum), IN PLACE, every chain in one launch.  v, momentum, grad: (C,3,D,H,W)
    float32 on the GPU, grad what a transition hands out as grad_v (sigma^2 already applied); sigma: the preconditioner field of
    that shape or None (= 1); eps: injected standard normals of that shape or None (the in-kernel Philox draw keyed by seed and
    iteration).  Returns (v, momentum)."""
    if v.dim() != 5 or v.shape[1] != 3:
        raise L.IrsError(f'v must have shape (C,3,D,H,W), got {tuple(v.shape)}')
    for name, t in (('momentum', momentum), ('grad', grad), ('sigma', sigma), ('eps', eps)):
        if t is not None and t.shape != v.shape:
            raise L.IrsError(f'{name} must have the shape of v {tuple(v.shape)}, got {tuple(t.shape)}')
    C, _, D, H, W = v.shape
    _call('irs_sghmc_update', L.dev_ptr(v, torch.float32), L.dev_ptr(momentum, torch.float32), L.dev_ptr(grad, torch.float32),
          L.dev_ptr(sigma, torch.float32, allow_none=True), L.dev_ptr(eps, torch.float32, allow_none=True), C, D, H, W, float(lr),
          float(friction), float(temperature), int(seed) & (2 ** 64 - 1), int(iteration) & (2 ** 64 - 1))
    return v, momentum


def kinetic_temperature(momentum, sigma, lr, friction):
    """Per chain mean(m^2 / (lr sigma^2)) (1 - friction / 2), a float64 tensor (C,).  Without a gradient the momentum is an AR(1)
    process with variance 2 friction lr T sigma^2 / (1 - (1 - friction)^2) = lr T sigma^2 / (1 - friction / 2): the reading is
    then T, whatever the friction, and about T while the step is small.  A reading far above T says lr is too large: the
    gradient's own contribution to the momentum is no longer small against the noise's.  A plain reduction; blocking only when
    the result is read."""
    m2 = momentum.to(torch.float64) ** 2
    if sigma is not None:
        m2 = m2 / sigma.to(torch.float64) ** 2
    return m2.flatten(1).mean(dim=1) * ((1.0 - 0.5 * float(friction)) / float(lr))


def _number(what, key, value):
    if isinstance(value, bool) or not isinstance(value, numbers.Real):
        raise ValueError(f'{what}.{key} must be a number, got {value!r}')
    return float(value)


def sampler_options(cfg_trainer):
    """`trainer.sampler = {"type": "SGHMC", "friction": 0.1, "temperature": 1.0}` -> {'type', 'friction', 'temperature'}, or None
    when the option is absent or its type is "SGLD" (and then nothing anywhere changes).  friction and temperature are optional;
    their defaults are choices for the user to tune, NOT measured optima.

    Refuses a value that is no dict, unknown keys, a missing or unknown type, friction / temperature next to "SGLD", wrong types
    (booleans as numbers too), friction outside (0, 1] and a temperature that is negative or not finite."""
    what = 'trainer.sampler'
    opt = cfg_trainer.get('sampler')
    if opt is None:
        return None
    if not isinstance(opt, dict):
        raise ValueError(f'{what} must be a dict with the keys {list(OPTION_KEYS)}, got {opt!r}')
    unknown = set(opt) - set(OPTION_KEYS)
    if unknown:
        raise ValueError(f'{what}: unknown keys {sorted(unknown)}; known: {list(OPTION_KEYS)}')
    kind = opt.get('type')
    if kind not in SAMPLERS:
        raise ValueError(f'{what}.type must be one of {list(SAMPLERS)}, got {kind!r}')
    if kind == 'SGLD':
        if len(opt) > 1:
            raise ValueError(f'{what}: {sorted(set(opt) - {"type"})} belong to "SGHMC"; the type is "SGLD"')
        return None
    friction = _number(what, 'friction', opt.get('friction', DEFAULT_FRICTION))
    temperature = _number(what, 'temperature', opt.get('temperature', DEFAULT_TEMPERATURE))
    _check_numbers(what + '.', friction, temperature)
    return {'type': kind, 'friction': friction, 'temperature': temperature}


def extra_optimizer_keys(cfg_optimizer):
    """the keys of `optimizer_SG_MCMC.args` other than `lr`, sorted: they are read by nobody (the update takes the learning rate
    and nothing else), which the trainer says once in its log"""
    return sorted(set(dict(cfg_optimizer.get('args', {}))) - {'lr'})
