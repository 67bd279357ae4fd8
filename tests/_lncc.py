"""fp64 restatement of the LNCC data term (csrc/lncc_kernels.hip; include/irsgmcmc.h: irs_lncc_fwd, irs_lncc_bwd) and the tolerance a
float32 evaluation of it is held to.  Plain torch, no GPU, the formulas written out with `box` / `box_t` of tests/_data_gradient.py: the
boxes are small matrices there, so nothing here shares the kernels' marching, their ring or their fold-the-padding weights.

    S_x = box(x) for x in F, M, F F, M M, F M                     n = (2r+1)^3
    A  = S_fm - S_f S_m / n     Bf = S_ff - S_f^2 / n     Bm = S_mm - S_m^2 / n     den = Bf Bm + eps     cc = A^2 / den     d = 1 - cc
    p = 2 u A / den             q = 2 u A^2 Bf / den^2    t = (q S_m - p S_f) / n
    g_M = M box^T(q) - F box^T(p) - box^T(t)                      ( = d/dM of sum u d )

The tolerance, derived on this side only (nothing of it comes from what the kernels return), to first order:

 1. A window sum of the forward kernel is 2r+1 products summed along x, 2r+1 such sums along y, 2r+1 plane sums along z:
    1 + 3 (2r+1) roundings, each at most U times a partial sum of absolute values, which the whole box of absolute values bounds.
    N = (2r+1)^2 + (2r+1) + 2, the count `tol_lcc` uses for a box summed plane by plane, is at least that for every r (10 <= 14,
    16 <= 32, 22 <= 58, 28 <= 92) and is kept:  e_S = N U box(|x|).
 2. Through A, Bf, Bm, den, r = A / den, p = 2 u r, q = p r Bf, d = 1 - A r and t = (q S_m - p S_f) / n, each by the derivative's
    absolute values plus U times the absolute addends for every operation of its own (the order the kernel evaluates them in).
 3. box^T of the adjoint kernel: per axis 2r+1 taps, each a multiplication by its fold weight and an addition: NT = 6 (2r+1)
    roundings, each at most U box^T(|c|).  So e_box^T(c) = box^T(e_c) + NT U box^T(|c|)  -- box^T with absolute values, which it has.
 4. g = (M bq - F bp) - bt and the scale: the three products' errors and 4 U of the absolute addends.

First order needs e_den well below den: `terms` refuses inputs where e_den > den / 4 (a flat window of a LARGE image; the test
images have texture everywhere), so no case can pass on a tolerance that blew up.
The sums are held to 1e-5 of sum |u| d, the project's loss tolerance (fp64 accumulation of float32 terms sits far inside it)."""
import torch

from tests import _data_gradient as G

F64 = torch.float64
U = G.U
EPS = 1e-5
LOSS_RTOL = 1e-5


def window_count(r):
    k = 2 * r + 1
    return k * k + k + 2


def adjoint_count(r):
    return 6 * (2 * r + 1)


def terms(fixed, moving, u, r, eps=EPS, dtype=F64):
    """fixed, moving, u: broadcastable (..., D, H, W) -> dict of S_f, S_m, S_ff, S_mm, S_fm, A, Bf, Bm, den, d, p, q, t in `dtype`,
    every step in the order of the kernel (r = A / den first)"""
    f, m, u = fixed.to(dtype), moving.to(dtype), torch.as_tensor(u).to(dtype)
    n = float((2 * r + 1) ** 3)
    S_f, S_m = G.box(f, r), G.box(m, r)
    S_ff, S_mm, S_fm = G.box(f * f, r), G.box(m * m, r), G.box(f * m, r)
    S_f, S_ff = torch.broadcast_tensors(S_f, S_m)[0], torch.broadcast_tensors(S_ff, S_m)[0]
    A = S_fm - S_f * S_m / n
    Bf = S_ff - S_f * S_f / n
    Bm = S_mm - S_m * S_m / n
    den = Bf * Bm + torch.tensor(eps, dtype=dtype)
    rr = A / den
    p = 2.0 * u * rr
    q = p * rr * Bf
    d = 1.0 - A * rr
    t = (q * S_m - p * S_f) / n
    return dict(S_f=S_f, S_m=S_m, S_ff=S_ff, S_mm=S_mm, S_fm=S_fm, A=A, Bf=Bf, Bm=Bm, den=den, r=rr, d=d, p=p, q=q, t=t)


def gradient(fixed, moving, p, q, t, r, drop=(), seam=None, no_t=False):
    """g_M from the coefficient maps.  The deliberate mistakes of the host test: drop / seam of G.box_t (a fold left out on a face, a
    ring not primed at a segment seam), no_t: the t term omitted"""
    f, m = fixed.to(p.dtype), moving.to(p.dtype)
    g = m * G.box_t(q, r, drop, seam) - f * G.box_t(p, r, drop, seam)
    return g if no_t else g - G.box_t(t, r, drop, seam)


def loss_sums(u, d):
    """sum u d per chain (leading axis) in float64"""
    return (torch.as_tensor(u).to(F64) * d.to(F64)).flatten(1).sum(1)


def autograd_gradient(fixed, moving, u, r, eps=EPS):
    """d/dM of sum u d through float64 autograd of the definition, no coefficient maps involved"""
    m = moving.detach().to(F64).clone().requires_grad_(True)
    f = fixed.to(F64)
    n = float((2 * r + 1) ** 3)
    S_f, S_m = G.box(f, r), G.box(m, r)
    A = G.box(f * m, r) - S_f * S_m / n
    den = (G.box(f * f, r) - S_f * S_f / n) * (G.box(m * m, r) - S_m * S_m / n) + eps
    loss = (torch.as_tensor(u).to(F64) * (1.0 - A * A / den)).sum()
    return torch.autograd.grad(loss, m)[0]


def tolerance(fixed, moving, u, r, eps=EPS, scale=1.0):
    """-> dict d, p, q, t, g: how far a float32 evaluation may be from the float64 one, per element (steps 1 to 4 of the module's
    docstring); `scale`: the factor the kernel multiplies g by (the weight of a transition)"""
    T = terms(fixed, moving, u, r, eps)
    f, m, ua = fixed.to(F64).abs(), moving.to(F64).abs(), torch.as_tensor(u).to(F64).abs()
    n = float((2 * r + 1) ** 3)
    N, NT = window_count(r), adjoint_count(r)
    e_f, e_m = N * U * G.box(f, r), N * U * G.box(m, r)
    e_ff, e_mm, e_fm = N * U * G.box(f * f, r), N * U * G.box(m * m, r), N * U * G.box(f * m, r)
    S_f, S_m, A, Bf, Bm, den, rr, p, q = (T[k].abs() for k in ('S_f', 'S_m', 'A', 'Bf', 'Bm', 'den', 'r', 'p', 'q'))
    e_A = e_fm + (S_m * e_f + S_f * e_m) / n + 3 * U * (T['S_fm'].abs() + S_f * S_m / n)
    e_Bf = e_ff + 2 * S_f * e_f / n + 3 * U * (T['S_ff'].abs() + S_f * S_f / n)
    e_Bm = e_mm + 2 * S_m * e_m / n + 3 * U * (T['S_mm'].abs() + S_m * S_m / n)
    e_den = Bm * e_Bf + Bf * e_Bm + 2 * U * (Bf * Bm + eps)
    if not bool((e_den <= den / 4).all()):
        raise ValueError('a window too flat for its intensities: the first-order tolerance does not hold (e_den > den / 4)')
    e_r = e_A / den + A * e_den / (den * den) + U * rr
    e_p = 2 * ua * e_r + 2 * U * p
    e_q = rr * Bf * e_p + p * Bf * e_r + p * rr * e_Bf + 2 * U * q
    e_d = rr * e_A + A * e_r + 2 * U * (1.0 + A * rr)
    e_t = (S_m * e_q + q * e_m + S_f * e_p + p * e_f) / n + 3 * U * (q * S_m + p * S_f) / n
    bt = lambda e, c: G.box_t(e, r) + NT * U * G.box_t(c.abs(), r)
    e_bp, e_bq, e_bt = bt(e_p, T['p']), bt(e_q, T['q']), bt(e_t, T['t'])
    bp, bq, btt = G.box_t(T['p'], r).abs(), G.box_t(T['q'], r).abs(), G.box_t(T['t'], r).abs()
    e_g = m * e_bq + f * e_bp + e_bt + 4 * U * (m * bq + f * bp + btt)
    return dict(d=e_d, p=e_p, q=e_q, t=e_t, g=abs(scale) * e_g)


def reference(fixed, moving, u, r, eps=EPS, scale=1.0):
    """what one call of the two operators has to return: dict d, p, q, t, g, sums (float64) and tol (dict, + sums)"""
    T = terms(fixed, moving, u, r, eps)
    out = {k: T[k] for k in ('d', 'p', 'q', 't')}
    out['g'] = scale * gradient(fixed, moving, T['p'], T['q'], T['t'], r)
    ub = torch.broadcast_tensors(torch.as_tensor(u).to(F64), T['d'])[0]
    out['sums'] = scale * loss_sums(ub, T['d'])
    out['tol'] = tolerance(fixed, moving, u, r, eps, scale)
    out['tol']['sums'] = LOSS_RTOL * abs(scale) * loss_sums(ub.abs(), T['d'].abs())
    return out


def float32_in_kernel_order(fixed, moving, u, r, eps=EPS):
    """the same formulas carried out in float32, operation by operation in the kernel's order -> dict d, p, q, t, g"""
    T = terms(fixed.to(torch.float32), moving.to(torch.float32), torch.as_tensor(u).to(torch.float32), r, eps, dtype=torch.float32)
    g = gradient(fixed.to(torch.float32), moving.to(torch.float32), T['p'], T['q'], T['t'], r)
    return dict(d=T['d'], p=T['p'], q=T['q'], t=T['t'], g=g)


def images(dims, C=1, raised=0.0, seed=5):
    """the images of the tests: `smooth_fixed` (blobs plus smooth noise, texture everywhere) raised by `raised`, per chain when C > 1,
    and the triangle-wave moving image scaled to 0..1.75 with a smooth per-chain ripple, so that the chains differ.
    -> fixed (C,1,D,H,W), moving (C,1,D,H,W) float32"""
    fixed, _ = G.smooth_fixed(dims, C)
    gen = torch.Generator().manual_seed(seed)
    moving = G.tri_image(dims) / 8.0 + 0.25 * torch.rand(C, 1, *dims, generator=gen)
    return (fixed + raised).to(torch.float32).contiguous(), moving.to(torch.float32).contiguous()
