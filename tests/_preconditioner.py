"""numpy restatement of the adaptive preconditioner (include/irsgmcmc.h: irs_precond_accumulate, irs_precond_sigma) with the
device's evaluation order: every float32 step one IEEE operation (numpy's float32 +, *, /, sqrt are correctly rounded, and none is
fused), the window sums and the two means in float64.  The window sum has the device's order (dz, dy, dx ascending); the order
of the two mean sums is free -- the tests compare them within the re-association bound and hand the device's own means back for
the field."""
import numpy as np

f32 = np.float32
SUMMARY_KEYS = ('s_mean', 'G_mean', 'sigma_min', 'sigma_max', 'sigma2_mean', 'clamped_low', 'clamped_high', 'nonfinite')


def accumulate(V, grad_v, sigma, beta):
    """V (1,3,D,H,W) float32, grad_v (C,3,D,H,W) float32, sigma like grad_v or None -> (the new V, the non-finite g counted)"""
    V, grad_v = np.asarray(V, f32), np.asarray(grad_v, f32)
    beta = f32(beta)
    omb = f32(1.0) - beta
    with np.errstate(all='ignore'):
        g = grad_v if sigma is None else grad_v / (np.asarray(sigma, f32) * np.asarray(sigma, f32))
        q = g[0] * g[0]
        for c in range(1, g.shape[0]):
            q = q + g[c] * g[c]
        m = q / f32(g.shape[0])
        new = (beta * V[0]) + (omb * m)
    assert new.dtype == f32
    return new[None], int((~np.isfinite(g)).sum())


def bias_correction(beta, count):
    return 1.0 if count < 1 else 1.0 / (1.0 - float(beta) ** int(count))


def corrected(V, bias, smooth):
    """vhat (3,D,H,W) float32: V * (float)bias, then the (2r+1)^3 box mean with replicate padding"""
    vhat = np.asarray(V, f32)[0] * f32(bias)
    r = int(smooth)
    if r == 0:
        return vhat
    pad = np.pad(vhat.astype(np.float64), ((0, 0), (r, r), (r, r), (r, r)), mode='edge')
    _, D, H, W = vhat.shape
    acc = np.zeros(vhat.shape, np.float64)
    for dz in range(2 * r + 1):
        for dy in range(2 * r + 1):
            for dx in range(2 * r + 1):
                acc = acc + pad[:, dz:dz + D, dy:dy + H, dx:dx + W]
    return (acc / float((2 * r + 1) ** 3)).astype(f32)


def means(V, bias, smooth, damping, sbar=None):
    """(sbar, Gbar) in float64, summed by numpy's pairwise sum.  sbar given: Gbar of the G formed with THAT sbar (lambda is
    rounded to float32, so the last bits of sbar can move every G)"""
    with np.errstate(all='ignore'):
        s = np.sqrt(corrected(V, bias, smooth))
        sbar = float(s.astype(np.float64).sum() / s.size) if sbar is None else float(sbar)
        G = _G(s, sbar, damping)
        return sbar, float(G.astype(np.float64).sum() / G.size)


def _G(s, sbar, damping):
    if sbar == 0.0:
        return np.ones_like(s)
    lam = f32(float(damping) * sbar)
    with np.errstate(all='ignore'):
        return f32(1.0) / (lam + s)


def sigma_field(V, C, bias, smooth, damping, sigma_min, sigma_max, sbar=None, gbar=None, nonfinite=0):
    """-> (sigma (C,3,D,H,W) float32, summary dict).  sbar / gbar: the two means to use (the device's own, for a bit-for-bit
    comparison of the field); None: this restatement's"""
    sbar, own_gbar = means(V, bias, smooth, damping, sbar)
    gbar = own_gbar if gbar is None else float(gbar)
    with np.errstate(all='ignore'):
        s = np.sqrt(corrected(V, bias, smooth))
        raw = np.sqrt(_G(s, sbar, damping) / f32(gbar))
        sg = np.minimum(np.maximum(raw, f32(sigma_min)), f32(sigma_max))
    assert sg.dtype == f32
    summary = {'s_mean': sbar, 'G_mean': gbar, 'sigma_min': float(sg.min()), 'sigma_max': float(sg.max()),
               'sigma2_mean': float((sg.astype(np.float64) ** 2).sum() / sg.size),
               'clamped_low': int((raw < f32(sigma_min)).sum()), 'clamped_high': int((raw > f32(sigma_max)).sum()),
               'nonfinite': int(nonfinite)}
    return np.broadcast_to(sg, (C, *sg.shape)).copy(), summary
