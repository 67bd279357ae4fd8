"""Data and regularisation losses with the reference's class names and constructor arguments (model/loss.py).

Volume work (the LCC map and its adjoint, the finite-difference energy) runs in the HIP kernels; what is left in torch
is scalar / K-vector arithmetic.  `Trainer._SGLD_transition` does not call these forward methods at all -- it hands the
objects' parameters to the fused engine -- but they keep the reference's call surface (`map`, `forward`, `log_pdf`,
`log_pdf_VD`, `init_parameters`, the properties, `reg_loss(v) -> (loss, log_y)`) usable on their own.
"""
import math
from abc import ABC, abstractmethod

import numpy as np
import torch
from torch import nn
from torch.nn.functional import log_softmax

from . import distributions as model_distr
from .. import bending as _bending
from .. import lncc as _lncc
from .. import mi as _mi
from .. import ngf as _ngf
from .. import ops as _ops
from ..utils.diff_op import DifferentialOperator, GradientOperator, HessianOperator


class DataLoss(nn.Module, ABC):
    @abstractmethod
    def forward(self, z):
        pass

    @abstractmethod
    def map(self, im_fixed, im_moving):
        pass


class _LCCMap(torch.autograd.Function):
    @staticmethod
    def forward(ctx, im_fixed, im_moving, s):
        fhat = _ops.lcc_normalise(im_fixed.contiguous(), s)
        z, sigma_m = _ops.lcc_map_fwd(fhat, im_moving.contiguous(), s)
        ctx.s = s
        ctx.save_for_backward(fhat, z, sigma_m)
        return z

    @staticmethod
    def backward(ctx, g_z):
        fhat, z, sigma_m = ctx.saved_tensors
        return None, _ops.lcc_map_bwd(fhat, z, sigma_m, g_z.contiguous(), ctx.s), None


class GMM(DataLoss):
    """zero-mean Gaussian mixture over the LCC-normalised residual (model/loss.py:38-114)"""

    def __init__(self, no_components, s):
        super().__init__()
        self.no_components = no_components
        self.logits = nn.Parameter(torch.zeros(no_components))
        self.log_std = nn.Parameter(torch.zeros(no_components))
        self.register_buffer('_log_sqrt_2pi', torch.tensor(0.5 * math.log(2.0 * math.pi)))
        self.s = s
        self.kernel_sz = s * 2 + 1
        self.sz = float(self.kernel_sz ** 3)

    @torch.no_grad()
    def init_parameters(self, sigma):
        sigma = float(sigma)
        self.log_std.data.copy_(torch.linspace(math.log(sigma / 100.0), math.log(sigma * 5.0), steps=self.no_components))

    @property
    def log_proportions(self):
        return log_softmax(self.logits + 1e-2, dim=0)

    @property
    def log_scales(self):
        return self.log_std

    @property
    def proportions(self):
        return torch.exp(self.log_proportions)

    @property
    def scales(self):
        return torch.exp(self.log_scales)

    @property
    def precision(self):
        return torch.exp(-2.0 * self.log_std)

    def log_pdf(self, z):
        E = 0.5 * (z.reshape(1, -1, 1) * torch.exp(-1.0 * self.log_std)) ** 2
        return torch.logsumexp((self.log_proportions - self.log_std - self._log_sqrt_2pi) - E, dim=-1)

    def log_pdf_VD(self, z_scaled):
        E = 0.5 * z_scaled ** 2
        return torch.logsumexp((self.log_proportions - self.log_std - self._log_sqrt_2pi) - E, dim=-1)

    def forward(self, z):
        return self.reduce(z)

    def map(self, im_fixed, im_moving):
        """z = LCC(F) - LCC(M) with (2s+1)^3 replicate-padded box statistics (HIP, LDS-tiled)"""
        if im_fixed.dim() == 5 and im_fixed.shape[0] > 1 and im_fixed.stride(0) == 0:
            im_fixed = im_fixed[:1]
        return _LCCMap.apply(im_fixed, im_moving, self.s)

    def reduce(self, z):
        return -1.0 * self.log_pdf(z).sum()


class SSD(DataLoss):
    """builder-defined sum of squared differences (BASELINE.json configs 1, 2, 4): z = F - M o phi,
    loss = 0.5 sum (z / sigma)^2.  No counterpart in the reference."""

    def __init__(self, sigma=0.1):
        super().__init__()
        self.sigma = float(sigma)
        self.no_components = 1

    def map(self, im_fixed, im_moving):
        return im_fixed - im_moving

    def forward(self, z):
        return 0.5 * torch.sum((z / self.sigma) ** 2)


class _LNCCMap(torch.autograd.Function):
    """d = 1 - cc of the two images; backward runs both HIP operators with the incoming gradient as the upstream weight"""

    @staticmethod
    def forward(ctx, im_fixed, im_moving, radius, eps):
        ctx.radius, ctx.eps = radius, eps
        ctx.save_for_backward(im_fixed, im_moving)
        return _lncc.lncc_forward(im_fixed, im_moving, radius, eps, want_coef=False, want_sums=False)['d']

    @staticmethod
    def backward(ctx, g_d):
        im_fixed, im_moving = ctx.saved_tensors
        coef = _lncc.lncc_forward(im_fixed, im_moving, ctx.radius, ctx.eps, upstream=g_d.contiguous(), want_map=False,
                                  want_sums=False)['coef']
        return None, _lncc.lncc_backward(im_fixed, im_moving, coef, ctx.radius), None, None


class LNCC(DataLoss):
    """local normalised cross-correlation over a (2 radius + 1)^3 box window, VoxelMorph's squared form: map = 1 - cc,
    loss = weight * sum map.  Insensitive to a local gain and offset of either image.  No counterpart in the reference."""

    def __init__(self, radius=2, weight=1.0, eps=1e-5):
        super().__init__()
        self.radius, self.weight, self.eps = int(radius), float(weight), float(eps)
        self.no_components = 1

    def map(self, im_fixed, im_moving):
        if im_fixed.dim() == 5 and im_fixed.shape[0] > 1 and im_fixed.stride(0) == 0:
            im_fixed = im_fixed[:1]
        return _LNCCMap.apply(im_fixed.contiguous(), im_moving.contiguous(), self.radius, self.eps)

    def forward(self, z):
        return self.weight * z.sum()


class _NGFMap(torch.autograd.Function):
    """the NGF distance map d of the two images; backward runs both HIP operators with the incoming gradient as the upstream weight"""

    @staticmethod
    def forward(ctx, im_fixed, im_moving, eps_f, eps_m):
        if im_fixed.requires_grad:
            raise NotImplementedError('NGF.map differentiates with respect to the moving image only: the fixed image must not require a '
                                      'gradient (it would silently receive none)')
        ctx.eps = eps_f, eps_m
        ctx.save_for_backward(im_fixed, im_moving)
        return _ngf.ngf_forward(im_fixed, im_moving, eps_f, eps_m, want_coef=False, want_sums=False)['d']

    @staticmethod
    def backward(ctx, g_d):
        im_fixed, im_moving = ctx.saved_tensors
        coef = _ngf.ngf_forward(im_fixed, im_moving, *ctx.eps, upstream=g_d.contiguous(), want_map=False, want_sums=False)['coef']
        return None, _ngf.ngf_backward(coef), None, None


class NGF(DataLoss):
    """normalised gradient field distance (Haber & Modersitzki 2006): map = 1 - (grad F . grad M)^2 / ((|grad F|^2 + fixed_eps^2)
    (|grad M|^2 + moving_eps^2)), loss = weight * sum map.  It compares the direction of the image gradients only, and not their
    sign: local, and free of a common contrast.  fixed_eps / moving_eps: the edge parameters, or None for `found_eps` -- the pair a
    caller computed once for the images at hand, as the trainer does -- and, without that, the mean of |grad I| over the whole
    volume of the images of the call (`ngf.ngf_edge_parameters`; a constant, not differentiated).  The gradient is with respect to
    the moving image only; a fixed image that requires one is refused.  No counterpart in the reference."""

    def __init__(self, weight=1.0, fixed_eps=None, moving_eps=None):
        super().__init__()
        self.weight = float(weight)
        self.fixed_eps = None if fixed_eps is None else float(fixed_eps)
        self.moving_eps = None if moving_eps is None else float(moving_eps)
        self.found_eps = None   # (eps_f, eps_m) computed for the pair at hand, used where the two above are None
        self.no_components = 1

    def map(self, im_fixed, im_moving):
        if im_fixed.dim() == 5 and im_fixed.shape[0] > 1 and im_fixed.stride(0) == 0:
            im_fixed = im_fixed[:1]
        eps_f, eps_m = self.fixed_eps, self.moving_eps
        if eps_f is None or eps_m is None:
            found = self.found_eps or _ngf.ngf_edge_parameters(im_fixed.detach(), im_moving.detach())
            eps_f, eps_m = found[0] if eps_f is None else eps_f, found[1] if eps_m is None else eps_m
        return _NGFMap.apply(im_fixed.contiguous(), im_moving.contiguous(), eps_f, eps_m)

    def forward(self, z):
        return self.weight * z.sum()


class _MILoss(torch.autograd.Function):
    """n * (ln B - MI) per chain (C,) float64; backward runs the gradient kernel with the incoming gradient as the per-chain scale"""

    @staticmethod
    def forward(ctx, im_fixed, im_moving, mask, bins, fixed_range, moving_range):
        out = _mi.mi_forward(im_fixed, im_moving, mask, bins, fixed_range, moving_range)
        ctx.bins, ctx.ranges, ctx.mask = bins, out['ranges'], mask
        ctx.save_for_backward(im_fixed, im_moving, out['table'])
        return out['stats'][:, 6].clone()

    @staticmethod
    def backward(ctx, g_loss):
        im_fixed, im_moving, table = ctx.saved_tensors
        g = _mi.mi_backward(im_fixed, im_moving, table, ctx.mask, ctx.bins, ctx.ranges[:2], ctx.ranges[2:],
                            scale=g_loss.to(torch.float32).contiguous())
        return None, g, None, None, None, None


class MI(DataLoss):
    """mutual information of the two images, a Mattes-style estimator (zero-order window on the fixed image, cubic B-spline window
    on the moving one, `bins` bins each): loss = weight * sum over the chains of n * (ln bins - MI) >= 0, n the voxels under the
    mask with both intensities finite.  Needs no common contrast of the two images.  fixed_range / moving_range: (lo, hi), or None
    for the min / max of the finite values (the fixed image under its mask, the moving image over the whole volume) at every call.
    No counterpart in the reference.  MI is NOT a per-voxel map followed by a masked sum -- the table ln(p_ab / (p_a p_b)) couples
    all voxels of a chain -- so `forward` takes the images and the mask, the base-class signature of the reference's DataLoss, and
    `map` / `reduce` raise."""

    def __init__(self, bins=32, weight=1.0, fixed_range=None, moving_range=None):
        super().__init__()
        self.bins, self.weight = int(bins), float(weight)
        self.fixed_range = None if fixed_range is None else tuple(float(x) for x in fixed_range)
        self.moving_range = None if moving_range is None else tuple(float(x) for x in moving_range)
        self.no_components = 1

    def forward(self, im_fixed, im_moving, mask=None):
        if im_fixed.dim() == 5 and im_fixed.shape[0] > 1 and im_fixed.stride(0) == 0:
            im_fixed = im_fixed[:1]
        if mask is not None and mask.dim() == 5 and mask.shape[0] > 1 and mask.stride(0) == 0:
            mask = mask[:1]
        terms = _MILoss.apply(im_fixed.contiguous(), im_moving.contiguous(), None if mask is None else mask.contiguous(), self.bins,
                              self.fixed_range, self.moving_range)
        return self.weight * terms.sum()

    def map(self, im_fixed, im_moving):
        raise NotImplementedError('MI is no per-voxel map followed by a masked sum: its table ln(p_ab / (p_a p_b)) is formed from the '
                                  'joint histogram of all masked voxels.  Call the loss itself: MI()(im_fixed, im_moving, mask)')

    def reduce(self, z):
        raise NotImplementedError('MI has no residual map to reduce (see MI.map): call the loss itself with the images and the mask')


class _Energy(torch.autograd.Function):
    """y_c = sum (replicate-padded forward differences)^2 (HIP reduction, fp64 accumulators); backward = 2 D^T D v"""

    @staticmethod
    def forward(ctx, v):
        ctx.save_for_backward(v)
        return _ops.reg_energy(v.contiguous()).to(v.dtype)

    @staticmethod
    def backward(ctx, g_y):
        v, = ctx.saved_tensors
        with torch.enable_grad():
            vv = v.detach().requires_grad_(True)
            y = torch.sum(GradientOperator()(vv) ** 2, dim=(1, 2, 3, 4, 5))
            g, = torch.autograd.grad(y, vv, g_y.to(y.dtype))
        return g


class _BendingEnergy(torch.autograd.Function):
    """y_c = sum (GradientOperator applied twice)^2, the bending energy; forward and backward (2 H^T W H v) both in HIP"""

    @staticmethod
    def forward(ctx, v):
        ctx.save_for_backward(v)
        return _bending.bending_energy(v).to(v.dtype)

    @staticmethod
    def backward(ctx, g_y):
        v, = ctx.saved_tensors
        return _bending.bending_energy_grad(v, g_y)


class RegLoss(nn.Module, ABC):
    """all regularisers are functions of the energy y = |D v|^2 (model/loss.py:122-169)"""

    def __init__(self, diff_op=None, dims=None, learnable=False):
        super().__init__()
        self.dims = dims
        self.dof = np.prod(dims) * 3.0
        self.learnable = learnable
        if diff_op is None:
            self.diff_op = DifferentialOperator()
        elif isinstance(diff_op, str):
            self.diff_op = DifferentialOperator.from_string(diff_op)
        elif isinstance(diff_op, DifferentialOperator):
            self.diff_op = diff_op
        else:
            self.diff_op = diff_op()

    def forward(self, input, *args, **kwargs):
        if isinstance(self.diff_op, GradientOperator):
            y = _Energy.apply(input)
        elif isinstance(self.diff_op, HessianOperator):
            y = _BendingEnergy.apply(input)
        else:
            y = torch.sum(self.diff_op(input) ** 2, dim=tuple(range(1, input.dim())))
        return self._loss(y, *args, **kwargs)

    @abstractmethod
    def _loss(self, y, *args, **kwargs):
        pass


class RegLoss_L2(RegLoss):
    """0.5 w y - 0.5 dof log w (model/loss.py:172-198)"""

    def __init__(self, w_reg, diff_op=None, dims=None, learnable=False):
        super().__init__(diff_op=diff_op, dims=dims, learnable=learnable)
        self.log_w_reg = nn.Parameter(torch.tensor(math.log(w_reg)), requires_grad=learnable)

    def _loss(self, y):
        return 0.5 * self.log_w_reg.exp() * y - 0.5 * self.dof * self.log_w_reg, y.log()


class RegLoss_Student(RegLoss):
    """model/loss.py:201-241"""

    def __init__(self, diff_op=None, dims=None, nu0=2e-6, lambda0=1e-6, a0=1e-6, b0=1e-6):
        super().__init__(diff_op=diff_op, dims=dims, learnable=False)
        self.a0 = nu0 / 2.0 if nu0 != 2e-6 else a0
        if lambda0 != 1e-6:
            b0 = self.a0 / lambda0
        self.b0_twice = b0 * 2.0

    def _loss(self, y):
        return torch.log(self.b0_twice + y) * (self.a0 + 0.5 * self.dof), y.log()


class RegLoss_EnergyBased(RegLoss):
    """-log p(y) + (dof/2 - 1) log y (model/loss.py:244-270)"""

    @abstractmethod
    def _mlog_energy_prior(self, y, *args, **kwargs):
        pass

    def _loss(self, y, *args, **kwargs):
        return self._mlog_energy_prior(y, *args, **kwargs) + (0.5 * self.dof - 1.0) * y.log(), y.log()


class RegLoss_LogNormal(RegLoss_EnergyBased):
    """log-normal prior on the energy; loc0 = E[expGamma(dof/2, w/2)], log_scale0 = log 4 + log loc0
    (model/loss.py:273-312)"""

    def __init__(self, w_reg=1.0, diff_op=None, dims=None, learnable=False):
        super().__init__(diff_op=diff_op, dims=dims, learnable=learnable)
        loc_init = model_distr.LogEnergyExpGammaPrior(w_reg, self.dof).expectation().clone().detach()
        self.loc = nn.Parameter(loc_init, requires_grad=learnable)
        self.log_scale = nn.Parameter(math.log(4.0) + loc_init.log(), requires_grad=learnable)
        self.w_reg = w_reg

    @property
    def scale(self):
        return self.log_scale.exp()

    def _mlog_energy_prior(self, y, *args, **kwargs):
        return y.log() + self.log_scale + 0.5 * ((y.log() - self.loc) / self.scale) ** 2


class RegLoss_LogNormal_L2(RegLoss_EnergyBased):
    """model/loss.py:315-321"""

    def __init__(self, w_reg, diff_op=None, dims=None):
        super().__init__(diff_op=diff_op, dims=dims, learnable=False)
        self.gamma_distr = model_distr._GammaDistribution(0.5 * self.dof, 0.5 * w_reg, learnable=False)

    def _mlog_energy_prior(self, y, *args, **kwargs):
        return -1.0 * self.gamma_distr(y.log())


class EntropyMultivariateNormal(nn.Module):
    """entropy terms of the VI stage (model/loss.py:342-372); out of the MCMC hot path, kept so that configs resolve"""

    def forward(self, **kwargs):
        log_var, u = kwargs['log_var'], kwargs['u']
        sigma = torch.exp(0.5 * log_var)
        if len(kwargs) == 2:
            return 0.5 * (torch.log1p(torch.sum(torch.pow(u / sigma, 2), dim=(1, 2, 3, 4))) + torch.sum(log_var, dim=(1, 2, 3, 4)))
        sample_n, u_n = (kwargs['sample'] - kwargs['mu']) / sigma, u / sigma
        t1 = torch.sum(torch.pow(sample_n, 2), dim=(1, 2, 3, 4))
        t2 = torch.pow(torch.sum(sample_n * u_n, dim=(1, 2, 3, 4)), 2) / (1.0 + torch.sum(torch.pow(u_n, 2), dim=(1, 2, 3, 4)))
        return 0.5 * (t1 - t2)
