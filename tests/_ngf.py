"""The NGF data term (csrc/ngf_kernels.hip, csrc/ngf_device.h; include/irsgmcmc.h: irs_ngf_fwd, irs_ngf_bwd) restated twice, and the
bound a float32 evaluation of it is held to.  Plain torch / numpy, no GPU.

    a = grad F, b = grad M      P = a.b      Nf = |a|^2 + eps_f^2      Nm = |b|^2 + eps_m^2
    r = P / (Nf Nm)     d = 1 - P r     s = P / Nm     k = -2 u r     c = k (a - s b)     g_M = grad^T c   ( = d/dM of sum u d )

 1. The definition in float64 torch (`terms`, `gradient`).  grad and grad^T are small DENSE MATRICES per axis (`grad_matrix`, its
    transpose), applied by tensordot: nothing here shares the kernels' marching, their register rings or their tap weights.
    `autograd_gradient` differentiates the definition itself, with the differences written as index_select's, no matrix and no
    coefficient map involved.
 2. The float32 numpy restatement in the operation order of ngf_device.h (`restate32`): every numpy float32 operation is rounded
    once, as every __f*_rn intrinsic is, so the operators are held to it BIT FOR BIT.

The bound between the two (`tolerance`), derived on this side only, to first order, with U = 2^-24 per rounded operation and the
absolute derivatives; the images are float32, so they carry no error of their own:

    a_i = 0.5 (hi - lo)               one rounding (the halving is exact)          e_a = U |a_i|
    P   = sum a_i b_i                 3 products, 2 additions                      e_P = sum (|b_i| e_a + |a_i| e_b) + 3 U sum |a_i b_i|
    Nf  = sum a_i^2 + eps^2           4 products, 3 additions, all terms >= 0      e_Nf = 2 sum |a_i| e_a + 5 U Nf          (Nm alike)
    den = Nf Nm                                                                    e_den = Nm e_Nf + Nf e_Nm + U den
    r   = P / den                                                                  e_r = e_P / den + |P| e_den / den^2 + U |r|
    d   = 1 - P r                                                                  e_d = |r| e_P + |P| e_r + 2 U (1 + |P r|)
    s   = P / Nm                                                                   e_s = e_P / Nm + |P| e_Nm / Nm^2 + U |s|
    k   = (-2 u) r                    (the doubling is exact)                      e_k = 2 |u| e_r + U |k|
    t_i = a_i - s b_i                                                              e_t = e_a + |b_i| e_s + |s| e_b + U (|a_i| + 2 |s b_i|)
    c_i = k t_i                                                                    e_c = |t_i| e_k + |k| e_t + U |c_i|
    g   = sum over the axes of 0.5 (sm cm - sp cp)      per axis one subtraction (the tap weights and the halving are exact), then
          two additions                                                            e_g = sum |G^T| e_c + 3 U sum |G^T| |c|
    and one more rounding U |scale g| where the transition multiplies by its weight.

First order needs e_den well below den: `tolerance` refuses inputs with e_den > den / 4, so no case passes on a bound that blew up.
The sums are held to 1e-5 of sum |u| d, the project's loss tolerance (float64 accumulation of float32 terms sits far inside it)."""
import numpy as np
import torch

F64 = torch.float64
U = 2.0 ** -24
LOSS_RTOL = 1e-5
AXES = (-3, -2, -1)  # z, y, x: the order every sum over the axes runs in

# the seeded mistakes of the host test (arguments of `gradient`)
MISTAKES = ('drop_fold_low', 'drop_fold_high', 'no_sb', 'swap_eps', 'flip_face')


def eps32(eps):
    """an edge parameter as the device holds it: rounded to float32 (both restatements start from that value)"""
    return float(np.float32(eps))


def grad_matrix(n):
    """(n, n) float64: the central difference with clamped indices on an axis of length n"""
    G = torch.zeros(n, n, dtype=F64)
    for y in range(n):
        G[y, min(y + 1, n - 1)] += 0.5
        G[y, max(y - 1, 0)] -= 0.5
    return G


def apply_axis(A, t, ax):
    """the matrix A applied along axis `ax` of t"""
    return torch.movedim(torch.tensordot(t, A, dims=([ax], [1])), -1, ax)


def adjoint_matrix(n, mistake=None):
    """grad^T on an axis of length n.  drop_fold_low / drop_fold_high: the replicated padding's fold left out of that face row (what
    grad^T of a ZERO-padded difference would give there); flip_face: the sign of the high face row flipped"""
    GT = grad_matrix(n).t().clone()
    if mistake == 'drop_fold_low':
        GT[0, 0] = 0.0
    elif mistake == 'drop_fold_high':
        GT[n - 1, n - 1] = 0.0
    elif mistake == 'flip_face':
        GT[n - 1] = -GT[n - 1]
    return GT


def image_gradient(im):
    """[a_z, a_y, a_x] of im (..., D, H, W) through the dense matrices"""
    return [apply_axis(grad_matrix(im.shape[ax]), im, ax) for ax in AXES]


def terms(fixed, moving, u, eps_f, eps_m, mistake=None):
    """fixed, moving, u: broadcastable (..., D, H, W) -> dict a, b (lists of three), P, Nf, Nm, r, d, s, k, c (list of three), float64"""
    f, m, u = fixed.to(F64), moving.to(F64), torch.as_tensor(u).to(F64)
    eps_f, eps_m = eps32(eps_f), eps32(eps_m)
    if mistake == 'swap_eps':
        eps_f, eps_m = eps_m, eps_f
    a, b = image_gradient(f), image_gradient(m)
    P = a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
    Nf = a[0] * a[0] + a[1] * a[1] + a[2] * a[2] + eps_f * eps_f
    Nm = b[0] * b[0] + b[1] * b[1] + b[2] * b[2] + eps_m * eps_m
    r = P / (Nf * Nm)
    d = 1.0 - P * r
    s = P / Nm
    k = -2.0 * u * r
    c = [k * (a[i] - (0.0 if mistake == 'no_sb' else s * b[i])) for i in range(3)]
    return dict(a=a, b=b, P=P, Nf=Nf, Nm=Nm, r=r, d=d, s=s, k=k, c=c)


def gradient(c, mistake=None, axis=-2):
    """g_M = grad^T c from the three coefficient maps; a face mistake is seeded on `axis` only"""
    g = 0.0
    for i, ax in enumerate(AXES):
        g = g + apply_axis(adjoint_matrix(c[i].shape[ax], mistake if ax == axis else None), c[i], ax)
    return g


def loss_sums(u, d):
    """sum u d per chain (leading axis) in float64"""
    ub = torch.broadcast_tensors(torch.as_tensor(u).to(F64), d.to(F64))[0]
    return (ub * d.to(F64)).flatten(1).sum(1)


def autograd_gradient(fixed, moving, u, eps_f, eps_m):
    """d/dM of sum u d through float64 autograd of the definition: differences by index_select, no matrix, no coefficient map"""
    m = moving.detach().to(F64).clone().requires_grad_(True)
    f = fixed.to(F64)
    eps_f, eps_m = eps32(eps_f), eps32(eps_m)

    def diff(im):
        out = []
        for ax in AXES:
            n = im.shape[ax]
            i = torch.arange(n)
            out.append(0.5 * (im.index_select(ax, (i + 1).clamp(max=n - 1)) - im.index_select(ax, (i - 1).clamp(min=0))))
        return out

    a, b = diff(f), diff(m)
    P = sum(x * y for x, y in zip(a, b))
    Nf = sum(x * x for x in a) + eps_f ** 2
    Nm = sum(y * y for y in b) + eps_m ** 2
    loss = (torch.as_tensor(u).to(F64) * (1.0 - P * P / (Nf * Nm))).sum()
    return torch.autograd.grad(loss, m)[0]


def tolerance(fixed, moving, u, eps_f, eps_m, scale=1.0):
    """-> dict d, c (list of three), g: how far a float32 evaluation may be from the float64 one, per element (the module's
    docstring); `scale`: the factor the adjoint kernel multiplies g by (the weight of a transition)"""
    T = terms(fixed, moving, u, eps_f, eps_m)
    ua = torch.as_tensor(u).to(F64).abs()
    a, b = [x.abs() for x in T['a']], [x.abs() for x in T['b']]
    P, Nf, Nm, r, s, k = (T[n].abs() for n in ('P', 'Nf', 'Nm', 'r', 's', 'k'))
    e_a, e_b = [U * x for x in a], [U * x for x in b]
    e_P = sum(b[i] * e_a[i] + a[i] * e_b[i] for i in range(3)) + 3 * U * sum(a[i] * b[i] for i in range(3))
    e_Nf = 2 * sum(a[i] * e_a[i] for i in range(3)) + 5 * U * Nf
    e_Nm = 2 * sum(b[i] * e_b[i] for i in range(3)) + 5 * U * Nm
    den = Nf * Nm
    e_den = Nm * e_Nf + Nf * e_Nm + U * den
    if not bool((e_den <= den / 4).all()):
        raise ValueError('the first-order tolerance does not hold (e_den > den / 4)')
    e_r = e_P / den + P * e_den / (den * den) + U * r
    e_d = r * e_P + P * e_r + 2 * U * (1.0 + P * r)
    e_s = e_P / Nm + P * e_Nm / (Nm * Nm) + U * s
    e_k = 2 * ua * e_r + U * k
    e_c, e_g, g_abs = [], 0.0, 0.0
    for i, ax in enumerate(AXES):
        t = (T['a'][i] - T['s'] * T['b'][i]).abs()
        e_t = e_a[i] + b[i] * e_s + s * e_b[i] + U * (a[i] + 2 * s * b[i])
        e_c.append(t * e_k + k * e_t + U * T['c'][i].abs())
        GT = grad_matrix(T['c'][i].shape[ax]).t().abs()
        e_g = e_g + apply_axis(GT, e_c[i], ax)
        g_abs = g_abs + apply_axis(GT, T['c'][i].abs(), ax)
    e_g = abs(scale) * (e_g + 3 * U * g_abs) + (U * abs(scale) * g_abs if scale != 1.0 else 0.0)
    return dict(d=e_d, c=e_c, g=e_g)


def reference(fixed, moving, u, eps_f, eps_m, scale=1.0):
    """what one call of the two operators has to return in float64: dict d, c (list), g, sums and tol (dict, + sums)"""
    T = terms(fixed, moving, u, eps_f, eps_m)
    out = dict(d=T['d'], c=T['c'], g=scale * gradient(T['c']), sums=scale * loss_sums(u, T['d']))
    out['tol'] = tolerance(fixed, moving, u, eps_f, eps_m, scale)
    out['tol']['sums'] = LOSS_RTOL * abs(scale) * loss_sums(torch.as_tensor(u).to(F64).abs(), T['d'].abs())
    return out


# ---------------------------------------------------------------- the float32 restatement, operation by operation (ngf_device.h)
F32 = np.float32


def _np32(t):
    return np.ascontiguousarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t, dtype=F32)


def _diff32(im, ax):
    n = im.shape[ax]
    i = np.arange(n)
    return F32(0.5) * (np.take(im, np.minimum(i + 1, n - 1), axis=ax) - np.take(im, np.maximum(i - 1, 0), axis=ax))


def _adjoint32(c, ax):
    n = c.shape[ax]
    i = np.arange(n)
    shape = [1] * c.ndim
    shape[ax] = n
    sm = np.where(i == 0, F32(-1), F32(1)).astype(F32).reshape(shape)
    sp = np.where(i == n - 1, F32(-1), F32(1)).astype(F32).reshape(shape)
    cm, cp = np.take(c, np.maximum(i - 1, 0), axis=ax), np.take(c, np.minimum(i + 1, n - 1), axis=ax)
    return F32(0.5) * (sm * cm - sp * cp)


def restate32(fixed, moving, u, eps_f, eps_m, scale=1.0):
    """fixed (1 or C,1,D,H,W), moving (C,1,D,H,W), u None or (1 or C,1,D,H,W) -> dict of torch float32 CPU tensors d (C,1,D,H,W),
    coef (C,3,D,H,W), g (C,1,D,H,W), ud (C,1,D,H,W) = fmul(u, d): what the two kernels return, bit for bit"""
    f, m = _np32(fixed), _np32(moving)
    uu = np.ones((1,) * m.ndim, dtype=F32) if u is None else _np32(u)
    a, b = [_diff32(f, ax) for ax in AXES], [_diff32(m, ax) for ax in AXES]
    ef2, em2 = F32(eps_f) * F32(eps_f), F32(eps_m) * F32(eps_m)
    dot = lambda p, q: (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]
    P = dot(a, b)
    Nf, Nm = dot(a, a) + ef2, dot(b, b) + em2
    r = P / (Nf * Nm)
    d = F32(1) - P * r
    s = P / Nm
    k = (F32(-2) * uu) * r
    c = [k * (a[i] - s * b[i]) for i in range(3)]
    g = (_adjoint32(c[0], -3) + _adjoint32(c[1], -2)) + _adjoint32(c[2], -1)
    if scale != 1.0:
        g = F32(scale) * g
    full = np.broadcast_to(d, m.shape)
    assert all(x.dtype == F32 for x in (P, Nf, Nm, r, d, s, k, g, *c))
    tt = lambda x: torch.from_numpy(np.broadcast_to(x, m.shape).copy())
    return dict(d=tt(full), coef=torch.cat([tt(x) for x in c], 1), g=tt(g), ud=tt(uu * full))


def images(dims, C=1, seed=5):
    """the images of the tests: uniform noise on a smooth ramp, texture everywhere, the chains different
    -> fixed (C,1,D,H,W), moving (C,1,D,H,W) float32"""
    gen = torch.Generator().manual_seed(seed)
    D, H, W = dims
    ramp = (torch.linspace(0, 1, D).view(D, 1, 1) + torch.linspace(0, 0.5, H).view(1, H, 1) - torch.linspace(0, 0.25, W).view(1, 1, W))
    fixed = torch.rand(C, 1, *dims, generator=gen) + ramp
    moving = 1.5 * torch.rand(C, 1, *dims, generator=gen) - 0.5 * ramp
    return fixed.to(torch.float32).contiguous(), moving.to(torch.float32).contiguous()


def upstream(dims, C=1, seed=9):
    """a random float upstream of both signs, (C,1,D,H,W) float32"""
    gen = torch.Generator().manual_seed(seed)
    return (2.0 * torch.rand(C, 1, *dims, generator=gen) - 1.0).to(torch.float32).contiguous()
