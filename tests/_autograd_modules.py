"""float64 restatements, inputs and tolerances for the torch-facing layer the VI stage runs through: the autograd Functions SGLD,
SobolevGrad (utils/functions.py), _SVFExp (utils/transformation.py), _Warp (utils/registration.py), _EnergyGrad (utils/diff_op.py),
_LCCMap, _Energy (model/loss.py), the RegLoss_* family and EntropyMultivariateNormal on top of them, and the raw gradient of one VI
iteration (trainer/vi.py) before Adam normalises it.  (_FFDUp is pinned bit for bit in tests/test_gpu_ffd.py.)  Plain torch on the
CPU; tests/test_autograd_modules_host.py proves what is here, tests/test_gpu_autograd_modules.py holds the layer to it.

The reference of every output is the CPU oracle (oracle/ops.py, oracle/transition.py) carried in float64 -- under
`default_dtype(float64)`, since the identity grid and a few constants take the default dtype.  Where a mistake has to be planted on
the reference side, the backward pass is restated explicitly (the cotangent assembly of _SVFExp, the transposed difference matrices
of _EnergyGrad, the per-chain g_y of _Energy, the antithetic mean of the VI loss) and the host test holds the restatement to plain
float64 autograd of the oracle ops.

Tolerances.  Two are closed forms: SGLD (4 U |value|: both sides make at most three roundings and one addition, and the velocity is
drawn with the sign of its noise term so that the sum does not cancel and |value| bounds every addend) and the LCC map's adjoint
(1e-5 A, the sum of the absolute addends, of tests/_data_gradient.py).  Every other one is MEASURED on the reference side: E is the
largest deviation, over the whole output, of the oracle run in float32 from the oracle run in float64 on the same inputs; the layer
gets 8 E (three bits for FMA contraction and another summation order), and never less than 2^-20 max|reference|.  Nothing here looks
at the code under test."""
import contextlib
import functools
import math
from collections import namedtuple

import torch

from oracle import OracleChain, OracleConfig
from oracle import ops as O
from oracle.transition import OracleVI, OracleVIConfig, entropy_terms
from tests import _data_gradient as G
from tests._report import check

F64, F32 = torch.float64, torch.float32
U = 2.0 ** -24            # unit roundoff of float32
MARGIN = 8.0              # the layer may be 8 E from float64
FLOOR = 2.0 ** -20        # ... and never has to be closer than this fraction of max|reference|
EXCLUDE_CAP = 1e-3        # _SVFExp only: the share of elements that may sit at a cell boundary (tests/test_gpu_ops.py)
TAU = 0.4
W_REG = 1.4
SHAPES = ((6, 9, 13), (10, 14, 22), (9, 17, 35))      # every extent different; (9, 17, 35) is wider than one 32-column stencil tile

Band = namedtuple('Band', 'ref E tol f32')            # reference (float64), measured E, tolerance, the float32 oracle's output


@contextlib.contextmanager
def default_dtype(dtype):
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def seed_of(dims, salt):
    return salt * 1000 + dims[0] * 169 + dims[1] * 13 + dims[2]


def smooth_field(C, dims, amp, seed):
    """as in tests/test_gpu_ops.py: white noise through the Sobolev kernel (float32)"""
    return O.separable_conv3d_replicate(amp * torch.randn(C, 3, *dims, generator=gen(seed)), O.sobolev_kernel_1d(3, 0.5)).contiguous()


def leaf(t, dtype):
    """a fresh leaf in `dtype`: the cached inputs themselves never take part in a graph"""
    return t.detach().to(dtype).clone().requires_grad_(True)


def _f64(t):
    return torch.as_tensor(t).detach().to(F64)


def measured(fn, *args, **kw):
    """fn(*args, dtype=...) -> {name: tensor}: run in float64 and in float32 -> {name: Band}"""
    r64, r32 = fn(*args, dtype=F64, **kw), fn(*args, dtype=F32, **kw)
    out = {}
    for k in r64:
        a, b = _f64(r64[k]), _f64(r32[k])
        E = float((a - b).abs().max())
        out[k] = Band(a, E, max(MARGIN * E, FLOOR * float(a.abs().max())), b)
    return out


def compare(test, name, got, band, cap=0.0):
    """hold `got` to band.tol of band.ref through check(), with E and the tolerance in the record's name.  cap > 0 (_SVFExp): up to
    that share of the elements may miss the tolerance and is left out of the check.  -> (deviation / tolerance, elements left out)"""
    got = _f64(got).cpu().reshape(band.ref.shape)
    bad = (got - band.ref).abs() > band.tol
    n_bad = int(bad.sum())
    if cap > 0.0 and 0 < n_bad <= cap * band.ref.numel():
        got = torch.where(bad, band.ref, got)
    else:
        n_bad = 0
    dev = check(test, f'{name} [E {band.E:.3e}]', got, band.ref, band.tol)
    return (dev / band.tol if band.tol > 0.0 else 0.0), n_bad


def units(got, ref, tol):
    """|got - ref| in units of a per-element tolerance; an element whose tolerance is 0 has to be exact"""
    dev = (_f64(got).cpu() - _f64(ref)).abs()
    tol = _f64(tol)
    return torch.where(tol > 0, dev / tol.clamp(min=1e-300), torch.where(dev == 0, torch.zeros_like(dev), torch.full_like(dev, float('inf'))))


def compare_units(test, name, got, ref, tol):
    """per-element tolerance: the record holds the worst deviation in units of it"""
    return check(test, name + ' [units of the tolerance]', units(got, ref, tol), torch.zeros(ref.shape, dtype=F64), 1.0)


# ------------------------------------------------------------------------------------------------------------------------------
# 1  SGLD
# ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sgld_case(dims, C=2):
    """sigma in [0.5, 1.5], injected eps, tau = 0.4; v has the sign of its noise term and |v| >= 0.5 (no cancellation: see above)"""
    g = gen(seed_of(dims, 1))
    eps = torch.randn(C, 3, *dims, generator=g)
    sigma = 0.5 + torch.rand(C, 3, *dims, generator=g)
    v = torch.where(eps < 0, -1.0, 1.0) * (0.5 + torch.randn(C, 3, *dims, generator=g).abs())
    cot = torch.randn(C, 3, *dims, generator=g)
    out = v.to(F64) + math.sqrt(2.0 * TAU) * sigma.to(F64) * eps.to(F64)
    grad = sgld_grad(sigma.to(F64), cot.to(F64))
    return {'v': v, 'sigma': sigma, 'eps': eps, 'cot': cot, 'out': out, 'grad': grad, 'tol_out': 4.0 * U * out.abs(), 'tol_grad': 4.0 * U * grad.abs()}


def sgld_grad(sigma, cot, mistake=None):
    return (sigma if mistake == 'sigma_for_sigma2' else sigma ** 2) * cot


# ------------------------------------------------------------------------------------------------------------------------------
# 2  SobolevGrad
# ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sobolev_case(dims, s, C=2):
    g = gen(seed_of(dims, 2) + s)
    return {'v': torch.randn(C, 3, *dims, generator=g), 'cot': torch.randn(C, 3, *dims, generator=g), 'taps': O.sobolev_kernel_1d(s, 0.5)}


def sobolev_oracle(dims, s, dtype=F64):
    c = sobolev_case(dims, s)
    return {'value': O.separable_conv3d_replicate(c['v'].to(dtype), c['taps'])}


# ------------------------------------------------------------------------------------------------------------------------------
# 3  _SVFExp
# ------------------------------------------------------------------------------------------------------------------------------
SVF_MODES = ('transformation', 'displacement', 'both')
# A voxel within rounding of a cell boundary at some step makes float32 and float64 pick different cells there, and the gradient
# jumps.  With 12 steps every voxel starts within |v| / 4096 of its own grid point, so a few near-zero velocities always flip and E
# holds their (small) jumps: a few 1e-3 of max|grad|.  With 4 steps nothing has to flip; one draw in three has an isolated voxel
# that does, which would blow E up a thousandfold and the tolerance with it.  These seeds have none: the host test holds the
# 4-step E to 4x the 99.9th percentile of the deviation, and every planted mistake to 100x the tolerance.
SVF_SEEDS = {(6, 9, 13): 3, (10, 14, 22): 0, (9, 17, 35): 3}


@functools.lru_cache(maxsize=None)
def svf_case(dims, C=2):
    """a smooth velocity of 1.5 voxels at its largest, smooth cotangents for the two outputs"""
    s = SVF_SEEDS[dims]
    v = smooth_field(C, dims, 1.0, 3000 + s)
    return {'v': (v * (1.5 / float(v.abs().max()))).contiguous(), 'g_t': smooth_field(C, dims, 1.0, 4000 + s),
            'g_disp': smooth_field(C, dims, 1.0, 5000 + s)}


def svf_cotangent(g_t, g_disp, dims, mistake=None):
    """what _SVFExp.backward hands to the adjoint of the squaring steps: dL/d(d_last) in normalised units.  transformation = id + d_last
    and displacement = d_last (n - 1) / 2 per channel (x <-> W, y <-> H, z <-> D); either cotangent may be None"""
    D, H, W = dims
    ref = g_t if g_t is not None else g_disp
    g = torch.zeros_like(ref) if g_t is None else g_t.clone()
    if g_disp is not None:
        n = (D, H, W) if mistake == 'scale_W_D_swapped' else (W, H, D)
        sc = torch.tensor([(k - 1) / 2.0 for k in n], dtype=ref.dtype).view(1, 3, 1, 1, 1)
        g = g + (g_disp if mistake == 'scale_left_out' else g_disp * sc)
    return g


def svf_oracle(dims, no_steps, mode, dtype=F64, mistake=None, plain=False):
    """-> transformation, displacement, grad_v.  plain: torch.autograd through the two outputs of O.svf_exp; otherwise the
    restatement: the cotangent assembled as above, pulled back through d_last"""
    c = svf_case(dims)
    with default_dtype(dtype):
        v = leaf(c['v'], dtype)
        g_t = c['g_t'].to(dtype) if mode in ('transformation', 'both') else None
        g_disp = c['g_disp'].to(dtype) if mode in ('displacement', 'both') else None
        t, disp, steps = O.svf_exp(v, no_steps, keep_steps=True)
        if plain:
            outs = [(o, g) for o, g in ((t, g_t), (disp, g_disp)) if g is not None]
            grad, = torch.autograd.grad([o for o, _ in outs], v, [g for _, g in outs])
        else:
            grad, = torch.autograd.grad(steps[-1], v, svf_cotangent(g_t, g_disp, dims, mistake))
    return {'transformation': t.detach(), 'displacement': disp.detach(), 'grad_v': grad}


@functools.lru_cache(maxsize=None)
def svf_bands(dims, no_steps, mode):
    return measured(svf_oracle, dims, no_steps, mode)


# ------------------------------------------------------------------------------------------------------------------------------
# 4  _Warp
# ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def warp_case(dims, C=2):
    """sampling position = voxel index + integer shift in {-1, 0, 1} + a fraction in {0.25, 0.375, .., 0.75}: never within 0.25 of a
    cell boundary, so no rounding of the float32 coordinate pipeline can change the cell.  Every other voxel of each face is pushed
    two voxels outward along that face's axis: the border clip then zeroes that channel of the gradient exactly.
    -> im (1,1,D,H,W), t (C,3,D,H,W) float32 normalised coordinates, p (float64 voxel positions), outside (C,3,D,H,W) bool, cot"""
    D, H, W = dims
    g = gen(seed_of(dims, 6))
    im = torch.rand(1, 1, D, H, W, generator=g)
    zz, yy, xx = torch.meshgrid(torch.arange(D), torch.arange(H), torch.arange(W), indexing='ij')
    idx = torch.stack((xx, yy, zz)).unsqueeze(0)                                  # channel 0 = x <-> W
    shift = torch.randint(-1, 2, (C, 3, D, H, W), generator=g)
    frac = 0.25 + 0.125 * torch.randint(0, 5, (C, 3, D, H, W), generator=g).to(F64)
    n = torch.tensor([W, H, D]).view(1, 3, 1, 1, 1)
    other = ((yy + zz) % 2 == 0, (xx + zz) % 2 == 0, (xx + yy) % 2 == 0)
    for ch in range(3):
        i = idx[0, ch]
        shift[:, ch] = torch.where((i == 0) & other[ch], torch.full_like(shift[:, ch], -2), shift[:, ch])
        shift[:, ch] = torch.where((i == n[0, ch] - 1) & other[ch], torch.full_like(shift[:, ch], 2), shift[:, ch])
    p = idx.to(F64) + shift.to(F64) + frac
    t = (2.0 * p / (n - 1).to(F64) - 1.0).to(F32).contiguous()
    outside = (p < 0) | (p > (n - 1).to(F64))
    return {'im': im, 't': t, 'p': p, 'outside': outside, 'n': n, 'cot': torch.randn(C, 1, D, H, W, generator=g)}


def warp_oracle(dims, dtype=F64):
    c = warp_case(dims)
    t = leaf(c['t'], dtype)
    warped = O.warp_trilinear(c['im'].to(dtype).expand(t.shape[0], -1, -1, -1, -1), t)
    grad, = torch.autograd.grad(warped, t, c['cot'].to(dtype))
    return {'warped': warped.detach(), 'grad_t': grad}


@functools.lru_cache(maxsize=None)
def warp_bands(dims):
    return measured(warp_oracle, dims)


# ------------------------------------------------------------------------------------------------------------------------------
# 5  _EnergyGrad
# ------------------------------------------------------------------------------------------------------------------------------
ENERGY_GRAD_SHAPES = ((6, 9, 13), (2, 6, 3))      # an extent of 2: the replicated last plane is the only difference there is


@functools.lru_cache(maxsize=None)
def energy_grad_case(dims, C=2):
    g = gen(seed_of(dims, 7))
    return {'v': torch.randn(C, 3, *dims, generator=g), 'cot': torch.randn(C, 3, *dims, 3, generator=g)}


def diff_matrix(n, dtype=F64, drop_last=False):
    """(M x)_i = x_{i+1} - x_i for i < n - 1; row n - 1 repeats row n - 2 (the DIFFERENCE array is replicate-padded)"""
    M = torch.zeros(n, n, dtype=dtype)
    for i in range(n - 1):
        M[i, i], M[i, i + 1] = -1.0, 1.0
    if not drop_last:
        M[n - 1] = M[n - 2]
    return M


def energy_grad_restated(v, cot, transformation, mistake=None):
    """nabla[:, a, ..., j] = M_a v[:, j] / sp_a and its adjoint sum_a M_a^T cot[:, a, ..., j] / sp_a, a = 0, 1, 2 <-> W, H, D"""
    D, H, W = v.shape[2:]
    sp = [2.0 / (W - 1), 2.0 / (H - 1), 2.0 / (D - 1)] if transformation else [1.0, 1.0, 1.0]
    sp_b = sp[::-1] if mistake == 'spacing_axes_swapped' else sp
    nabla, grad = torch.zeros(*v.shape[:1], 3, D, H, W, 3, dtype=v.dtype), torch.zeros_like(v)
    for a, ax in enumerate((-1, -2, -3)):
        M = diff_matrix(v.shape[ax], v.dtype)
        Mb = diff_matrix(v.shape[ax], v.dtype, drop_last=mistake == 'last_plane_dropped')
        for j in range(3):
            nabla[:, a, ..., j] = G.apply_axis(M, v[:, j], ax) / sp[a]
            grad[:, j] += G.apply_axis(Mb.t(), cot[:, a, ..., j], ax) / sp_b[a]
    return nabla, grad


def energy_grad_oracle(dims, transformation, dtype=F64):
    c = energy_grad_case(dims)
    v = leaf(c['v'], dtype)
    nabla = O.forward_differences(v, transformation)
    grad, = torch.autograd.grad(nabla, v, c['cot'].to(dtype))
    return {'nabla': nabla.detach(), 'grad_v': grad}


@functools.lru_cache(maxsize=None)
def energy_grad_bands(dims, transformation):
    return measured(energy_grad_oracle, dims, transformation)


# ------------------------------------------------------------------------------------------------------------------------------
# 6  _Energy and the RegLoss_* family
# ------------------------------------------------------------------------------------------------------------------------------
REG_CASES = ('l2_fixed', 'l2_learnable', 'student', 'lognormal_fixed', 'lognormal_learnable', 'lognormal_l2')
REG_SHAPES = ((6, 9, 13), (9, 17, 35))


def dof_of(dims):
    return float(dims[0] * dims[1] * dims[2]) * 3.0


@functools.lru_cache(maxsize=None)
def reg_case(dims, C=3):
    """three chains whose fields differ in amplitude by factors of 4: every chain has its own g_y"""
    g = gen(seed_of(dims, 8))
    amp = torch.tensor([1.0, 4.0, 16.0]).view(C, 1, 1, 1, 1)
    return {'v': (smooth_field(C, dims, 1.0, seed_of(dims, 9)) * amp).contiguous(), 'cot_loss': 0.5 + torch.rand(C, generator=g),
            'cot_log_y': torch.randn(C, generator=g)}


def reg_parameters(case, dims):
    """the learnable (or fixed) parameters of a case as the oracle initialises them -> {name: 0-dim tensor}"""
    if case.startswith('l2'):
        return {'log_w_reg': torch.tensor(math.log(W_REG), dtype=F32).to(F64)}       # (the module's parameter is float32)
    if case in ('lognormal_fixed', 'lognormal_learnable'):
        loc, log_scale = O.reg_lognormal_init(W_REG, dof_of(dims))
        return {'loc': loc.to(F64), 'log_scale': log_scale.to(F64)}
    return {}


def reg_loss_fn(case, dims, y, p):
    dof = dof_of(dims)
    if case.startswith('l2'):
        return O.reg_l2(y, p['log_w_reg'], dof)
    if case == 'student':
        return O.reg_student(y, dof, *O.student_params())
    if case == 'lognormal_l2':
        return O.reg_lognormal_l2(y, W_REG, dof)
    return O.reg_lognormal(y, p['loc'], p['log_scale'], dof)


def reg_oracle(case, dims, dtype=F64, mistake=None, plain=False):
    """-> loss, log_y (C,), grad_v, and grad_<name> of every parameter of a learnable case.  plain: torch.autograd through
    O.reg_energy and the loss; otherwise g_y = d total / d y is formed per chain first and pulled back through the energy"""
    c = reg_case(dims)
    learn = case.endswith('learnable')
    with default_dtype(dtype):
        v = leaf(c['v'], dtype)
        p = {k: t.to(dtype).requires_grad_(learn) for k, t in reg_parameters(case, dims).items()}
        wl, wy = c['cot_loss'].to(dtype), c['cot_log_y'].to(dtype)
        y = O.reg_energy(v)
        lp = list(p.values()) if learn else []
        if plain:
            loss, log_y = reg_loss_fn(case, dims, y, p)
            grads = torch.autograd.grad((wl * loss).sum() + (wy * log_y).sum(), [v] + lp)
            g_v, g_p = grads[0], grads[1:]
        else:
            y_leaf = y.detach().requires_grad_(True)
            loss, log_y = reg_loss_fn(case, dims, y_leaf, p)
            grads = torch.autograd.grad((wl * loss).sum() + (wy * log_y).sum(), [y_leaf] + lp)
            g_y, g_p = grads[0], grads[1:]
            if mistake == 'g_y_of_chain_0':
                g_y = g_y[:1].expand_as(g_y)
            g_v, = torch.autograd.grad(y, v, g_y)
    out = {'loss': loss.detach(), 'log_y': log_y.detach(), 'grad_v': g_v}
    if learn:
        out.update({'grad_' + k: g for k, g in zip(p, g_p)})
    return out


@functools.lru_cache(maxsize=None)
def reg_bands(case, dims):
    return measured(reg_oracle, case, dims)


# ------------------------------------------------------------------------------------------------------------------------------
# 7  _LCCMap (the kernel is pinned in tests/test_gpu_data_gradient.py: the wiring only)
# ------------------------------------------------------------------------------------------------------------------------------
LCC_SHAPES = ((6, 9, 13), (10, 14, 22))


@functools.lru_cache(maxsize=None)
def lcc_case(dims, s, C=2):
    """-> fixed (1,1,D,H,W), moving, g_z (C,1,D,H,W) float32; z, grad_moving in float64 through autograd of G.lcc_stats; tol_z as
    G.forward adds it up, tol_grad = 1e-5 A with A the absolute addends of the adjoint (G.lcc_adjoint)"""
    g = gen(seed_of(dims, 10) + s)
    fixed = torch.rand(1, 1, *dims, generator=g)
    moving = torch.rand(C, 1, *dims, generator=g)
    g_z = torch.randn(C, 1, *dims, generator=g)
    m = leaf(moving, F64)
    wh, sigma, _ = G.lcc_stats(m, s)
    z = G.lcc_stats(fixed.to(F64), s)[0] - wh
    grad, = torch.autograd.grad(z, m, g_z.to(F64))
    A = torch.stack([G.lcc_adjoint(g_z[c, 0].to(F64), wh[c, 0].detach(), sigma[c, 0].detach(), s)[1] for c in range(C)]).unsqueeze(1)
    tol_z = G.tol_lcc(fixed, s)[0] + G.tol_lcc(moving, s)[0] + U * z.detach().abs()
    return {'fixed': fixed, 'moving': moving, 'g_z': g_z, 'z': z.detach(), 'grad_moving': grad, 'tol_z': tol_z, 'tol_grad': 1e-5 * A}


# ------------------------------------------------------------------------------------------------------------------------------
# 8  EntropyMultivariateNormal
# ------------------------------------------------------------------------------------------------------------------------------
ENTROPY_NAMES = ('mu', 'log_var', 'u', 'sample')


@functools.lru_cache(maxsize=None)
def entropy_case(dims, C=2):
    g = gen(seed_of(dims, 11))
    shape = (C, 3, *dims)
    mu, log_var, u = 0.02 * torch.randn(shape, generator=g), -4.0 + 0.1 * torch.randn(shape, generator=g), 0.05 * torch.randn(shape, generator=g)
    sample = mu + torch.randn(shape, generator=g) * torch.exp(0.5 * log_var) + torch.randn(C, 1, 1, 1, 1, generator=g) * u
    return {'mu': mu, 'log_var': log_var, 'u': u, 'sample': sample, 'cot': 0.5 + torch.rand(C, generator=g)}


def entropy_oracle(dims, form, dtype=F64):
    """form 'log_det': entropy_terms(None, None, log_var, u); form 'sample': entropy_terms(sample, mu, log_var, u)"""
    c = entropy_case(dims)
    names = ('log_var', 'u') if form == 'log_det' else ENTROPY_NAMES
    p = {k: leaf(c[k], dtype) for k in names}
    value = entropy_terms(p.get('sample'), p.get('mu'), p['log_var'], p['u'])
    grads = torch.autograd.grad(value, list(p.values()), c['cot'].to(dtype))
    return {'value': value.detach(), **{'grad_' + k: g for k, g in zip(p, grads)}}


@functools.lru_cache(maxsize=None)
def entropy_bands(dims, form):
    return measured(entropy_oracle, dims, form)


# ------------------------------------------------------------------------------------------------------------------------------
# C  the gradient of the first VI iteration
# ------------------------------------------------------------------------------------------------------------------------------
VI_CASES = {
    'lognormal_learnable_vd_s2': {'dims': (11, 14, 19), 'reg_loss': 'RegLoss_LogNormal', 'learnable': True, 'vd': True, 'sobolev_s': 2, 'seed': 0},
    'l2_fixed_s3': {'dims': (13, 10, 17), 'reg_loss': 'RegLoss_L2', 'learnable': False, 'vd': False, 'sobolev_s': 3, 'seed': 1},
}
VI_FIELDS = ('mu', 'log_var', 'u')
NORM_RTOL = 1e-4          # ||g|| / ||g_ref|| per field


def vi_param_names(case):
    c = VI_CASES[case]
    if not c['learnable']:
        return ()
    return ('loc', 'log_scale') if c['reg_loss'] == 'RegLoss_LogNormal' else ('log_w_reg',)


@functools.lru_cache(maxsize=None)
def vi_case(case):
    """the set-up of tests/test_gpu_vi_fuzz.py: a synthetic pair, one chain, injected eps and x -> float32 CPU tensors"""
    from ir_sgmcmc_amd.data_loader import synthetic_pair
    c = VI_CASES[case]
    dims = c['dims']
    f1, m1 = synthetic_pair(dims, seed=c['seed'])
    g = gen(c['seed'])
    shape = (1, 3, *dims)
    vp0 = {'mu': 0.02 * torch.randn(shape, generator=g), 'log_var': torch.full(shape, -4.0) + 0.1 * torch.randn(shape, generator=g),
           'u': 0.05 * torch.randn(shape, generator=g)}
    return {'fixed': {'im': f1['im'].unsqueeze(0), 'mask': f1['mask'].unsqueeze(0)}, 'moving': {'im': m1['im'].unsqueeze(0)}, 'vp0': vp0,
            'eps': torch.randn(shape, generator=g), 'x': torch.randn(1, 1, 1, 1, 1, generator=g)}


def vi_oracle_config(case):
    c = VI_CASES[case]
    return OracleConfig(dims=c['dims'], no_chains=1, sobolev_s=c['sobolev_s'], uniform_noise=None, virtual_decimation=c['vd'],
                        reg_loss=c['reg_loss'], reg_learnable=c['learnable'], w_reg=W_REG)


def vi_oracle(case, dtype=F64, mistake=None, plain=False):
    """-> grad_mu, grad_log_var, grad_u (1,3,D,H,W) and grad_<name> of the learnable regulariser parameters, of the first iteration.
    plain: what OracleVI.step computes and returns under 'grads'; otherwise the loss is put together here from OracleVI.sample_loss
    (trainer.py:131-170), which is where the antithetic mean can be got wrong"""
    c = vi_case(case)
    cfg = vi_oracle_config(case)
    with default_dtype(dtype):
        fixed = {'im': c['fixed']['im'].to(dtype), 'mask': c['fixed']['mask']}
        moving = {'im': c['moving']['im'].to(dtype)}
        ch = OracleChain(cfg, v0=torch.zeros(1, 3, *cfg.dims))
        ch.init_gmm(fixed, moving)
        vi = OracleVI(ch, {k: t.to(dtype) for k, t in c['vp0'].items()}, OracleVIConfig())
        eps, x = c['eps'].to(dtype), c['x'].to(dtype)
        if plain:
            grads = vi.step(fixed, moving, eps, x)['grads']
        else:
            vp = vi.vp
            pert = eps * torch.exp(0.5 * vp['log_var']) + x * vp['u']
            t1 = vi.sample_loss(fixed, moving, vp['mu'] + pert, None)[0]
            t2 = vi.sample_loss(fixed, moving, vp['mu'] - pert, None)[0]
            if mistake == 'one_sample':
                t2 = t1
            mean = lambda k: (t1[k] + t2[k]) / 2.0
            data = mean('data') - ch.gmm_prior_terms()
            reg = mean('reg')
            if cfg.reg_learnable and cfg.reg_loss == 'RegLoss_LogNormal':
                reg = reg - mean('reg_loc_prior') - O.normal_log_pdf(ch.log_scale, *cfg.reg_scale_prior).sum()
            elif cfg.reg_learnable:
                reg = reg - mean('w_reg_prior')
            entropy = mean('entropy') + entropy_terms(None, None, vp['log_var'], vp['u']).sum()
            params = [vp[k] for k in VI_FIELDS] + ([p for g in ch.adam_reg.groups for p in g['params']] if ch.adam_reg is not None else [])
            grads = torch.autograd.grad(data + reg - entropy, params)
            if mistake == 'doubled':
                grads = [2.0 * g for g in grads]
    return {'grad_' + k: g.detach() for k, g in zip(VI_FIELDS + vi_param_names(case), grads)}


@functools.lru_cache(maxsize=None)
def vi_bands(case):
    return measured(vi_oracle, case)


def norm_ratio(got, ref):
    return float(_f64(got).norm()) / float(_f64(ref).norm())
