"""The mutual-information data term (include/irsgmcmc.h: irs_mi_fwd, irs_mi_bwd) restated in numpy float64, in exactly the operations
of the definition: the fixed bin in float32 (tests/_image_similarity.bin_index), the moving coordinate, the four Parzen weights and
their Q30 fixed point in float64 with every operation rounded once -- numpy contracts nothing -- and the histogram in exact uint64
integers (np.add.at).  The device has to reproduce the histogram bit for bit; T, MI, the data term, the gradient g and the pmi map
are held per element to tolerances DERIVED here from the float32 rounding of the table and of the outputs.

`reference_one(..., mistake=...)` seeds one of three mistakes into the gradient: 'tap_offset' (taps k0 .. k0 + 3 in place of k0 - 1 ..
k0 + 2), 'no_inside' (the gradient not zeroed where the moving coordinate was clamped) and 'pb_unnormalised' (T' = ln(p_ab / p_b) in
place of ln(p_ab / (p_a p_b)) -- which changes NOTHING while the derivative weights sum to zero, the row constant ln p_a cancels --
together with weights that do not: the last tap left out of the sum)."""
import math

import numpy as np

from tests._image_similarity import bin_index

F32, F64, U64 = np.float32, np.float64, np.uint64
Q = 30
EPS32 = 2.0 ** -24  # relative rounding error of a float32
MISTAKES = ('tap_offset', 'no_inside', 'pb_unnormalised')


def moving_scale(m_lo, m_hi, bins):
    return F64(bins - 3) / (F64(F32(m_hi)) - F64(F32(m_lo)))


def coords(m, m_lo, m_hi, bins):
    """m float32, finite -> (k0 int64, u float64 in [0, 1], inside bool)"""
    t_raw = (m.astype(F64) - F64(F32(m_lo))) * moving_scale(m_lo, m_hi, bins) + F64(1.0)
    t = np.minimum(np.maximum(t_raw, 1.0), F64(bins - 2))
    k0 = np.minimum(np.floor(t).astype(np.int64), bins - 3)
    return k0, t - k0.astype(F64), (t_raw >= 1.0) & (t_raw <= bins - 2)


def weights(u):
    om, u2 = 1.0 - u, u * u
    u3 = u2 * u
    a3, b3 = 3.0 * u3, 3.0 * u2
    return np.stack([((om * om) * om) / 6.0, ((a3 - 6.0 * u2) + 4.0) / 6.0, (((b3 - a3) + 3.0 * u) + 1.0) / 6.0, u3 / 6.0])


def weight_derivatives(u):
    om, u2 = 1.0 - u, u * u
    c = 1.5 * u2
    return np.stack([-((om * om) * 0.5), c - 2.0 * u, (u - c) + 0.5, u2 * 0.5])


def fixed_point(w, q_bits=Q):
    """(4, n) uint64: q_j = rint(w_j 2^Q) for j = 0, 2, 3 and q_1 the rest of 2^Q"""
    one = F64(2.0 ** q_bits)
    q = np.rint(w * one).astype(U64)
    q[1] = U64(1 << q_bits) - q[0] - q[2] - q[3]
    return q


def reference_one(f, m, mask, bins, f_range, m_range, weight=1.0, q_bits=Q, mistake=None):
    """one chain: f, m float32 arrays of one shape, mask bool of that shape or None -> dict; g, pmi and their tolerances have the
    shape of the images"""
    shape = f.shape
    f, m = np.asarray(f, F32).reshape(-1), np.asarray(m, F32).reshape(-1)
    masked = np.ones(f.size, bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    finite = np.isfinite(f) & np.isfinite(m)
    take = masked & finite
    idx = np.flatnonzero(take)
    n = idx.size
    a, f_out = bin_index(f[idx], f_range[0], f_range[1], bins)
    k0, u, inside = coords(m[idx], m_range[0], m_range[1], bins)
    w, dw = weights(u), weight_derivatives(u)
    q = fixed_point(w, q_bits)
    hist = np.zeros((bins, bins), U64)
    for j in range(4):
        np.add.at(hist, (a, k0 - 1 + j), q[j])
    rows, cols = hist.sum(axis=1, dtype=U64), hist.sum(axis=0, dtype=U64)
    total = int(rows.sum(dtype=U64))
    assert total == n << q_bits
    T = np.zeros((bins, bins), F64)
    out = {'hist': hist, 'rows': rows, 'counts_a': np.bincount(a, minlength=bins), 'n': n, 'n_nonfinite': int((masked & ~finite).sum()),
           'n_clipped': int((f_out | ~inside).sum()), 'take': take.reshape(shape)}
    if n:
        N = F64(total)
        p, pa, pb = hist.astype(F64) / N, rows.astype(F64) / N, cols.astype(F64) / N
        some = hist > 0
        with np.errstate(divide='ignore', invalid='ignore'):
            ratio = p / (pb[None, :] if mistake == 'pb_unnormalised' else pa[:, None] * pb[None, :])
        T[some] = np.log(ratio[some])
        mi = float(math.fsum((p * T).reshape(-1)))
        ent = lambda x: -float(math.fsum(x[x > 0] * np.log(x[x > 0])))
        out.update(mi=mi, h_fixed=ent(pa), h_moving=ent(pb), data_term=weight * n * (math.log(bins) - mi),
                   # a few ulp per term (two divisions, a log, a product) and a sum of B^2 terms in another order
                   tol_mi=8.0 * bins * bins * 2.0 ** -53 * float((p * (np.abs(T) + 1.0)).sum()),
                   # the same for the two marginal entropies: B terms -p ln p each (a division, a log, a product)
                   tol_h_fixed=8.0 * bins * 2.0 ** -53 * float((pa[pa > 0] * (np.abs(np.log(pa[pa > 0])) + 1.0)).sum()),
                   tol_h_moving=8.0 * bins * 2.0 ** -53 * float((pb[pb > 0] * (np.abs(np.log(pb[pb > 0])) + 1.0)).sum()))
    else:
        out.update(mi=0.0, h_fixed=0.0, h_moving=0.0, data_term=0.0, tol_mi=0.0, tol_h_fixed=0.0, tol_h_moving=0.0)
    out['tol_term'] = weight * n * out['tol_mi'] + 4 * 2.0 ** -53 * abs(out['data_term'])
    out['T'] = T
    out['tol_T'] = EPS32 * np.abs(T) + 2.0 ** -48 * (np.abs(T) + 1.0)  # its float32 rounding, and the device's own log
    scale = float(moving_scale(m_range[0], m_range[1], bins))
    shift = 0 if mistake != 'tap_offset' else 1
    taps = np.stack([T[a, np.minimum(k0 - 1 + j + shift, bins - 1)] for j in range(4)]) if n else np.zeros((4, 0))
    last = 3 if mistake == 'pb_unnormalised' else 4
    gate = np.ones(n, bool) if mistake == 'no_inside' else inside
    g, pmi = np.zeros(f.size, F64), np.zeros(f.size, F64)
    out.update(pmi_q_sum=0.0, pmi_q_bound=0.0)
    tol_g, tol_pmi = np.zeros(f.size, F64), np.zeros(f.size, F64)
    if n:
        g[idx] = -weight * scale * gate * (dw[:last] * taps[:last]).sum(axis=0)
        pmi[idx] = (w * taps).sum(axis=0)
        # the same sum with the weights the histogram received, q_j / 2^Q: THEIR total is n MI exactly; the w_j differ from them by
        # at most 2^-(Q+1) (three times that for q_1, which takes the rest), which bounds what sum pmi may miss n MI by
        out['pmi_q_sum'] = float(math.fsum(((q.astype(F64) / F64(2.0 ** q_bits)) * taps).reshape(-1)))
        out['pmi_q_bound'] = float((np.array([1.0, 3.0, 1.0, 1.0])[:, None] * 2.0 ** -(q_bits + 1) * np.abs(taps)).sum())
        # every T_j rounded to float32 (relative EPS32; the + 1 for the device's float64 sum of four terms and its log), the
        # result rounded to float32 once more.  The Q30 term is zero: the restatement forms T from the same integers.
        tol_g[idx] = weight * scale * (np.abs(dw) * EPS32 * (np.abs(taps) + 1.0)).sum(axis=0) + EPS32 * np.abs(g[idx])
        tol_pmi[idx] = (w * EPS32 * (np.abs(taps) + 1.0)).sum(axis=0) + EPS32 * np.abs(pmi[idx])
    out.update(g=g.reshape(shape), pmi=pmi.reshape(shape), tol_g=tol_g.reshape(shape), tol_pmi=tol_pmi.reshape(shape),
               inside=np.zeros(f.size, bool).reshape(shape))
    out['inside'].reshape(-1)[idx] = inside
    return out


def reference(fixed, moving, mask, bins, f_range, m_range, weight=1.0, mistake=None):
    """fixed (1 or C,1,D,H,W), moving (C,1,D,H,W) float32 arrays, mask (1 or C,1,D,H,W) or None -> list of reference_one per chain"""
    C = moving.shape[0]
    return [reference_one(fixed[c if fixed.shape[0] > 1 else 0, 0], moving[c, 0],
                          None if mask is None else mask[c if mask.shape[0] > 1 else 0, 0], bins, f_range, m_range, weight, Q, mistake)
            for c in range(C)]


def loss_one(f, m, mask, bins, f_range, m_range, q_bits=Q):
    """n (ln B - MI) of one chain for float64 moving intensities (the finite differences perturb m below float32 resolution):
    the definition again, with m taken as float64"""
    f = np.asarray(f, F32).reshape(-1)
    m = np.asarray(m, F64).reshape(-1)
    take = (np.ones(f.size, bool) if mask is None else np.asarray(mask).reshape(-1) != 0) & np.isfinite(f) & np.isfinite(m)
    a, _ = bin_index(f[take], f_range[0], f_range[1], bins)
    t_raw = (m[take] - F64(F32(m_range[0]))) * moving_scale(m_range[0], m_range[1], bins) + 1.0
    t = np.minimum(np.maximum(t_raw, 1.0), F64(bins - 2))
    k0 = np.minimum(np.floor(t).astype(np.int64), bins - 3)
    w = weights(t - k0)
    if q_bits is None:  # real weights
        hist = np.zeros((bins, bins), F64)
        for j in range(4):
            np.add.at(hist, (a, k0 - 1 + j), w[j])
        p = hist / hist.sum()
    else:
        q = fixed_point(w, q_bits)
        hist = np.zeros((bins, bins), U64)
        for j in range(4):
            np.add.at(hist, (a, k0 - 1 + j), q[j])
        p = hist.astype(F64) / F64(int(hist.sum(dtype=U64)))
    pa, pb = p.sum(axis=1), p.sum(axis=0)
    some = p > 0
    mi = float(math.fsum((p[some] * np.log(p[some] / (pa[:, None] * pb[None, :])[some]))))
    return take.sum() * (math.log(bins) - mi)


def pair(shape, C, seed, Cf=1, invert=True):
    """a correlated pair in [0, 1]: fixed (Cf,1,*shape) and moving (C,1,*shape) float32, the moving images a noisy, inverted copy"""
    rng = np.random.default_rng(seed)
    fixed = rng.random((Cf, 1, *shape)).astype(F32)
    noise = rng.random((C, 1, *shape)).astype(F32)
    base = F32(1.0) - fixed if invert else fixed
    return fixed, (F32(0.8) * base + F32(0.2) * noise).astype(F32)
