"""`TransitionEngine`: Python owner of one `irs_ctx` (include/irsgmcmc.h) -- the fused SG-MCMC transition.

This is what `Trainer._SGLD_transition` (ir_sgmcmc_amd/trainer/trainer.py) drives.  All tensors stay on the GPU; the
hyper-parameters (GMM, regulariser, Adam moments) live in a small device struct and are only copied to the host when
somebody asks for them (`state()`, `scalars()`), so a transition needs no host synchronisation at all.
"""
import ctypes as C
import math
from dataclasses import dataclass, field
from typing import Optional, Sequence, Tuple

import torch
from scipy.special import digamma

from . import _lib as L
from .ops import control_grid_size, sobolev_kernel_1d


@dataclass
class EngineConfig:
    """Flat mirror of the config.json keys the transition depends on (configs/*/config.json of the reference)."""
    dims: Tuple[int, int, int]
    no_chains: int = 1
    cps: Optional[Tuple[int, int, int]] = None          # transformation_module: SVFFD_3D args.cps
    no_steps: int = 12
    sobolev_s: int = 3                                    # Sobolev_grad.s (0 = disabled)
    sobolev_lambda: float = 0.5
    lr: float = 0.4                                       # optimizer_SG_MCMC.args.lr
    uniform_noise: float = 0.1                            # trainer.uniform_noise.magnitude (0 = disabled)
    virtual_decimation: bool = True
    data_loss: str = 'GMM'                                # 'GMM' (reference) | 'SSD' (builder-defined) | 'LNCC' (lcc_s = window radius) | 'MI' | 'NGF'
    gmm_components: int = 4
    lcc_s: int = 1
    ssd_sigma: float = 0.1
    lncc_weight: float = 1.0                              # 'LNCC': data term = lncc_weight * sum mask * (1 - cc), cc with + lncc_eps
    lncc_eps: float = 1e-5
    mi_bins: int = 32                                     # 'MI': data term = mi_weight * n * (ln mi_bins - MI); the bins travel in lcc_s
    mi_weight: float = 1.0
    mi_fixed_range: Optional[Tuple[float, float]] = None  # (lo, hi) of the two images; while either is None the engine waits for
    mi_moving_range: Optional[Tuple[float, float]] = None  # mi_set, and refuses a transition before it: no range is guessed
    ngf_weight: float = 1.0                               # 'NGF': data term = ngf_weight * sum mask * d (ngf.py); lcc_s is not read
    ngf_fixed_eps: Optional[float] = None                 # the two edge parameters; while either is None the engine waits for
    ngf_moving_eps: Optional[float] = None                # ngf_set, and refuses a transition before it: no eps is guessed
    gmm_lr_log_std: float = 0.2
    gmm_lr_logits: float = 0.2
    gmm_lr_decay: float = 0.001
    scale_prior: Tuple[float, float] = (0.0, 2.3)
    dirichlet_alpha: Sequence[float] = field(default_factory=lambda: [0.5])
    reg_loss: str = 'RegLoss_L2'   # 'RegLoss_L2' | 'RegLoss_LogNormal' | 'RegLoss_Student' | 'RegLoss_LogNormal_L2'
    w_reg: float = 1.4
    student: Tuple[float, float] = (1e-6, 2e-6)          # RegLoss_Student (a0, 2 b0), model/loss.py:224-232
    reg_learnable: bool = False
    reg_lr: Tuple[float, float] = (0.01, 0.01)
    reg_lr_decay: float = 0.001
    loc_prior_nu: float = 1.0
    loc_prior_w_reg: Optional[float] = None
    reg_scale_prior: Tuple[float, float] = (2.8, 5.0)
    seed: int = 0
    diff_op: str = 'GradientOperator'                     # reg_loss diff_op: 'GradientOperator' | 'HessianOperator' (bending energy)
    sampler: str = 'SGLD'                                 # 'SGLD' (the reference's scheme) | 'SGHMC' (sghmc.py: momentum, noise kept in v)
    sghmc_friction: float = 0.1                           # 'SGHMC': in (0, 1]; 1 = Langevin dynamics with persisted noise
    sghmc_temperature: float = 1.0                        # 'SGHMC': >= 0; 0 = no noise, a heavy-ball optimiser

    @property
    def dims_v(self):
        return control_grid_size(self.dims, self.cps) if self.cps else tuple(self.dims)

    @property
    def dof(self):
        return float(self.dims[0] * self.dims[1] * self.dims[2]) * 3.0  # parse_config.py:120,128


def lognormal_init(w_reg, dof, nu=1.0):
    """loc0 = digamma(nu dof / 2) - log(nu w / 2), log_scale0 = log 4 + log loc0 (model/loss.py:298-303)."""
    loc = float(digamma(0.5 * nu * dof)) - math.log(0.5 * nu * w_reg)
    return loc, math.log(4.0) + math.log(loc)


DATA_LOSSES = {'GMM': L.IRS_DATA_GMM_LCC, 'SSD': L.IRS_DATA_SSD, 'LNCC': L.IRS_DATA_LNCC, 'MI': L.IRS_DATA_MI, 'NGF': L.IRS_DATA_NGF}
DIFF_OPS = {'GradientOperator': L.IRS_DIFF_GRADIENT, 'HessianOperator': L.IRS_DIFF_HESSIAN}


def diff_op_code(name):
    """IRS_DIFF_* of a differential operator's class name"""
    if name not in DIFF_OPS:
        raise ValueError(f'diff_op {name!r} is not wired into the fused transition: one of {sorted(DIFF_OPS)}')
    return DIFF_OPS[name]


def irs_config(cfg: EngineConfig):
    """EngineConfig -> the C struct of include/irsgmcmc.h"""
    c = L.IrsConfig()
    c.diff_op = diff_op_code(cfg.diff_op)
    c.dims[:] = list(cfg.dims)
    c.cps[:] = list(cfg.cps) if cfg.cps else [0, 0, 0]
    c.no_chains, c.no_steps = cfg.no_chains, cfg.no_steps
    c.sobolev_s = cfg.sobolev_s or 0
    if c.sobolev_s:
        k = sobolev_kernel_1d(cfg.sobolev_s, cfg.sobolev_lambda)
        for i, x in enumerate(k):
            c.sobolev_kernel[i] = float(x)
    c.lr = cfg.lr
    c.uniform_alpha = cfg.uniform_noise or 0.0
    c.virtual_decimation = int(cfg.virtual_decimation)
    if cfg.data_loss not in DATA_LOSSES:
        raise ValueError(f'data_loss {cfg.data_loss!r} is not wired into the fused transition: one of {sorted(DATA_LOSSES)}')
    c.data_loss = DATA_LOSSES[cfg.data_loss]
    c.lcc_s, c.gmm_components, c.ssd_sigma = cfg.mi_bins if cfg.data_loss == 'MI' else cfg.lcc_s, cfg.gmm_components, cfg.ssd_sigma
    c.gmm_lr_log_std, c.gmm_lr_logits, c.gmm_lr_decay = cfg.gmm_lr_log_std, cfg.gmm_lr_logits, cfg.gmm_lr_decay
    c.adam_beta1, c.adam_beta2, c.adam_eps = 0.9, 0.999, 1e-8
    c.scale_prior_loc, c.scale_prior_scale = cfg.scale_prior
    conc = list(cfg.dirichlet_alpha)
    if len(conc) == 1:
        conc = conc * cfg.gmm_components
    for i, x in enumerate(conc):
        c.dirichlet_concentration[i] = float(x)
    c.reg_loss = {'RegLoss_L2': L.IRS_REG_L2, 'RegLoss_LogNormal': L.IRS_REG_LOGNORMAL, 'RegLoss_Student': L.IRS_REG_STUDENT,
                  'RegLoss_LogNormal_L2': L.IRS_REG_LOGNORMAL_L2}[cfg.reg_loss]
    c.reg_learnable = int(cfg.reg_learnable)
    c.w_reg, c.dof = cfg.w_reg, cfg.dof
    c.reg_lr0, c.reg_lr1, c.reg_lr_decay = cfg.reg_lr[0], cfg.reg_lr[1], cfg.reg_lr_decay
    c.loc_prior_nu = cfg.loc_prior_nu
    c.loc_prior_w_reg = cfg.w_reg if cfg.loc_prior_w_reg is None else cfg.loc_prior_w_reg
    c.reg_scale_prior_loc, c.reg_scale_prior_scale = cfg.reg_scale_prior
    shape = 0.5 * cfg.dof  # parse_config.py:136-140
    c.w_reg_prior_shape, c.w_reg_prior_rate = shape, 1.0 / shape
    if cfg.reg_loss == 'RegLoss_Student':
        c.w_reg_prior_shape, c.w_reg_prior_rate = float(cfg.student[0]), float(cfg.student[1])
    c.seed = cfg.seed
    return c


def _on_device(fn):
    """run a method with the engine's device current (launches go to the stream of THAT device)"""
    import functools

    @functools.wraps(fn)
    def wrapped(self, *a, **k):
        with torch.cuda.device(self.device):
            return fn(self, *a, **k)
    return wrapped


class TransitionEngine:
    def __init__(self, cfg: EngineConfig, device='cuda:0'):
        self.cfg = cfg
        self.device = torch.device(device)
        self.lib = L.load()
        self._c = c = irs_config(cfg)
        with torch.cuda.device(self.device):
            self._ctx = self._create(c)
        self._keep = {}
        if cfg.data_loss == 'LNCC':  # (irs_config has no room for the two: they travel in a call of their own)
            self.lncc_set(cfg.lncc_weight, cfg.lncc_eps)
        if cfg.data_loss == 'MI' and cfg.mi_fixed_range is not None and cfg.mi_moving_range is not None:
            self.mi_set(cfg.mi_weight, cfg.mi_fixed_range, cfg.mi_moving_range)
        if cfg.data_loss == 'NGF' and cfg.ngf_fixed_eps is not None and cfg.ngf_moving_eps is not None:
            self.ngf_set(cfg.ngf_weight, cfg.ngf_fixed_eps, cfg.ngf_moving_eps)
        # SGHMC: the momentum lives here, bound to the context before its first transition (irs_config has no room for the sampler)
        if cfg.sampler not in ('SGLD', 'SGHMC'):
            raise ValueError(f'sampler {cfg.sampler!r}: one of SGLD, SGHMC')
        self.momentum = None
        if cfg.sampler == 'SGHMC':
            self._bind_momentum()
        if cfg.reg_loss == 'RegLoss_LogNormal':
            st = self.state()
            st.reg_param[0], st.reg_param[1] = lognormal_init(cfg.w_reg, cfg.dof)
            self.set_state(st)

    def _stream(self):
        """the engine's device's current stream (not the current device's: an engine on cuda:1 stays there)"""
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _create(self, c):
        ctx = C.c_void_p()
        L.check(self.lib.irs_create(C.byref(c), C.byref(ctx)))
        return ctx

    def lncc_set(self, weight, eps):
        """irs_lncc_set: weight and eps of the LNCC data term; only before the first transition"""
        L.check(self.lib.irs_lncc_set(self._ctx, float(weight), float(eps)))

    def ngf_set(self, weight, fixed_eps, moving_eps):
        """irs_ngf_set: weight and the two edge parameters of the NGF data term; required, and only before the first transition"""
        L.check(self.lib.irs_ngf_set(self._ctx, float(weight), float(fixed_eps), float(moving_eps)))

    def mi_set(self, weight, fixed_range, moving_range):
        """irs_mi_set: weight and the two intensity ranges (lo, hi) of the MI data term; required, and only before the first
        transition"""
        (f_lo, f_hi), (m_lo, m_hi) = fixed_range, moving_range
        L.check(self.lib.irs_mi_set(self._ctx, float(weight), float(f_lo), float(f_hi), float(m_lo), float(m_hi)))

    def _bind_momentum(self):
        """irs_sghmc_set: a zeroed momentum (C, 3, *dims_v) that the transitions update next to v; only before the first one"""
        cfg = self.cfg
        momentum = torch.zeros((cfg.no_chains, 3, *cfg.dims_v), device=self.device, dtype=torch.float32)
        L.check(self.lib.irs_sghmc_set(self._ctx, float(cfg.sghmc_friction), float(cfg.sghmc_temperature), L.dev_ptr(momentum, torch.float32)))
        self.momentum = momentum

    def __del__(self):
        ctx, self._ctx = getattr(self, '_ctx', None), None
        if ctx:
            try:
                self.lib.irs_destroy(ctx)
            except Exception:
                pass

    def option(self, name, value):
        """a tuning / test switch of THIS context (include/irsgmcmc.h: irs_option_set)"""
        L.option_set(name, value, self._ctx)

    @_on_device
    def flush(self):
        """irs_flush: wait for the enqueued transitions and re-run those that ended as no-ops because a kernel-variant (slab:
        ghost-width) prediction failed; afterwards v / state / scalars are those of a chain that never mispredicted.  Call it
        before reading `v` at the end of a run (state() and scalars() call it themselves)."""
        L.check(self.lib.irs_flush(self._ctx, self._stream()))

    @property
    def recovered_transitions(self):
        n = C.c_uint64()
        L.check(self.lib.irs_recovered_transitions(self._ctx, C.byref(n)))
        return int(n.value)

    def set_sparse_adjoint(self, on):
        """irs_sparse_adjoint_set: False -> the adjoint squaring steps march full columns (the same numbers; A/B and parity runs)"""
        L.check(self.lib.irs_sparse_adjoint_set(self._ctx, int(bool(on))))

    @_on_device
    def sparse_adjoint(self):
        """irs_sparse_adjoint_get: per adjoint step k and chain c of the last transition, [k][c] = dict(engaged, piece_len, pieces,
        run_planes) -- whether the step marched only the planes the gradient reaches, and how they were cut"""
        n, ch = self.cfg.no_steps, self.cfg.no_chains
        buf = (C.c_int32 * (n * ch * 4))()
        L.check(self.lib.irs_sparse_adjoint_get(self._ctx, buf, self._stream()))
        keys = ('engaged', 'piece_len', 'pieces', 'run_planes')
        return [[dict(zip(keys, buf[(k * ch + c) * 4:(k * ch + c) * 4 + 4])) for c in range(ch)] for k in range(n)]

    def set_sparse_data(self, on):
        """irs_sparse_data_set: False -> warp, LCC map, statistics and data term run over the whole volume (the same numbers); an
        int n >= 2 -> on whatever the volume's size, with pieces of at most n planes (tests)"""
        L.check(self.lib.irs_sparse_data_set(self._ctx, int(on)))

    @_on_device
    def sparse_data(self):
        """irs_sparse_data_get: per kernel of the data stage and chain c of the last transition, [kernel][c] = dict(engaged,
        piece_len, pieces, run_planes); kernel in ('warp', 'map', 'stats', 'data_term')"""
        ch = self.cfg.no_chains
        buf = (C.c_int32 * (4 * ch * 4))()
        L.check(self.lib.irs_sparse_data_get(self._ctx, buf, self._stream()))
        keys = ('engaged', 'piece_len', 'pieces', 'run_planes')
        return {name: [dict(zip(keys, buf[(k * ch + c) * 4:(k * ch + c) * 4 + 4])) for c in range(ch)]
                for k, name in enumerate(('warp', 'map', 'stats', 'data_term'))}

    def set_sparse_forward(self, on):
        """irs_sparse_forward_set: False -> the forward squaring steps march the whole volume (the same numbers); an int n >= 2 -> on
        whatever the volume's size, with pieces of at most n planes (tests)"""
        L.check(self.lib.irs_sparse_forward_set(self._ctx, int(on)))

    @_on_device
    def sparse_forward(self):
        """irs_sparse_forward_get: per forward step k and chain c of the last transition, [k][c] = dict(engaged, piece_len, pieces,
        run_planes, width) -- whether the step computed only what a later kernel reads, how its columns were cut, its planned width"""
        n, ch = self.cfg.no_steps, self.cfg.no_chains
        buf = (C.c_int32 * (n * ch * 5))()
        L.check(self.lib.irs_sparse_forward_get(self._ctx, buf, self._stream()))
        keys = ('engaged', 'piece_len', 'pieces', 'run_planes', 'width')
        return [[dict(zip(keys, buf[(k * ch + c) * 5:(k * ch + c) * 5 + 5])) for c in range(ch)] for k in range(n)]

    def set_sparse_plan(self, reuse):
        """irs_sparse_plan_set: bit 0 -> piece lists whose inputs did not change are kept (default); 0 -> every list is rebuilt in every
        transition; bit 1 -> the adjoint's lists always from the extents of g_warped (A/B and parity runs)"""
        L.check(self.lib.irs_sparse_plan_set(self._ctx, int(reuse)))

    @_on_device
    def sparse_plan(self):
        """irs_sparse_plan_get: per family in ('data', 'forward', 'adjoint') dict(rebuilds, reuses): lists since the context was made"""
        buf = (C.c_int32 * 6)()
        L.check(self.lib.irs_sparse_plan_get(self._ctx, buf, self._stream()))
        return {name: dict(rebuilds=int(buf[2 * i]), reuses=int(buf[2 * i + 1])) for i, name in enumerate(('data', 'forward', 'adjoint'))}

    # ---------------------------------------------------------------- small state
    @property
    def workspace_bytes(self):
        return int(self.lib.irs_workspace_bytes(self._ctx))

    @_on_device
    def state(self):
        st = L.IrsState()
        L.check(self.lib.irs_get_state(self._ctx, C.byref(st), self._stream()))
        return st

    @_on_device
    def set_state(self, st):
        L.check(self.lib.irs_set_state(self._ctx, C.byref(st), self._stream()))

    @_on_device
    def scalars(self):
        sc = L.IrsScalars()
        L.check(self.lib.irs_get_scalars(self._ctx, C.byref(sc), self._stream()))
        n = self.cfg.no_chains
        return {k: [getattr(sc, k)[i] for i in range(n)] for k in ('alpha', 'data_term', 'reg_term', 'reg_energy', 'n_mask')}

    # ---------------------------------------------------------------- data
    def _io(self, fixed, moving, v, sigma=None, eps=None, unif=None, outputs=None):
        io = L.IrsIO()
        f_im, m_im, mask = fixed['im'], moving['im'], fixed['mask']
        io.fixed_im, io.moving_im = L.dev_ptr(f_im, torch.float32), L.dev_ptr(m_im, torch.float32)
        io.mask = L.dev_ptr(mask, torch.bool)
        io.fixed_chains, io.moving_chains, io.mask_chains = f_im.shape[0], m_im.shape[0], mask.shape[0]
        io.v = L.dev_ptr(v, torch.float32, allow_none=True)
        io.sigma = L.dev_ptr(sigma, torch.float32, allow_none=True)
        io.eps = L.dev_ptr(eps, torch.float32, allow_none=True)
        io.unif = L.dev_ptr(unif, torch.float32, allow_none=True)
        for k in ('curr_state', 'im_moving_warped', 'residuals', 'displacement', 'transformation', 'grad_v'):
            t = (outputs or {}).get(k)
            setattr(io, k, L.dev_ptr(t, torch.float32, allow_none=True))
        return io

    @staticmethod
    def _base(t):
        """`fixed['im'].expand(C, ...)` views (trainer.py:361-362) share one volume: hand the library the (1,...) base."""
        if t.dim() == 5 and t.stride(0) == 0 and t.shape[0] > 1:
            t = t[:1]
        return t.contiguous()

    @_on_device
    def prepare(self, fixed, moving):
        """Normalise dict inputs (collapse expanded chains) and pre-normalise the fixed image for the LCC map."""
        fixed = {k: self._base(v) for k, v in fixed.items() if k in ('im', 'mask')}
        moving = {k: self._base(v) for k, v in moving.items() if k in ('im',)}
        self._keep['fixed'], self._keep['moving'] = fixed, moving
        L.check(self.lib.irs_set_fixed(self._ctx, L.dev_ptr(fixed['im'], torch.float32), fixed['im'].shape[0],
                                       self._stream()))
        return fixed, moving

    @_on_device
    def gmm_init(self, fixed, moving, v_sample=None, warm_up=25):
        """Trainer.__GMM_init (trainer.py:529-547)."""
        io = self._io(fixed, moving, None)
        L.check(self.lib.irs_gmm_init(self._ctx, C.byref(io), L.dev_ptr(v_sample, torch.float32, allow_none=True),
                                      warm_up, self._stream()))

    @_on_device
    def transition(self, fixed, moving, v, sigma=None, eps=None, unif=None, outputs=None, timed=False):
        """One `_SGLD_transition`; updates `v` in place.  outputs: dict of preallocated tensors to fill."""
        io = self._io(fixed, moving, v, sigma, eps, unif, outputs)
        if timed:
            tm = L.IrsTimings()
            L.check(self.lib.irs_transition_timed(self._ctx, C.byref(io), self._stream(), C.byref(tm)))
            return {n: getattr(tm, n) for n, _ in tm._fields_}
        L.check(self.lib.irs_transition(self._ctx, C.byref(io), self._stream()))
        return None
