"""float64 numpy restatement of the split ESS and MCSE estimator ("Split ESS and MCSE"), computed from
full sample arrays; shared by the host and GPU tests."""
import math

import numpy as np


def split_sequences(samples):
    """samples (C, N, ...) -> (2C, n, ...) float64: half 0 = samples 0 .. N//2 - 1, half 1 = the last N//2 of every chain"""
    samples = np.asarray(samples, dtype=np.float64)
    N = samples.shape[1]
    n = N // 2
    return np.concatenate([samples[:, :n], samples[:, N - n:]], axis=0)


def var_plus_np(samples):
    """(n - 1) / n W + B / n per trailing element, as R-hat has it"""
    seqs = split_sequences(samples)
    n = seqs.shape[1]
    W = seqs.var(axis=1, ddof=1).mean(axis=0)
    B_n = seqs.mean(axis=1).var(axis=0, ddof=1)
    return (n - 1) / n * W + B_n


def variogram_np(samples, max_lag):
    """S_t = sum over sequences j and i = t+1 .. n of (psi_{i,j} - psi_{i-t,j})^2 for t = 1 .. max_lag -> (max_lag, ...);
    lags t >= n have no pairs and stay 0 (the device's vsum keeps max_lag slots)"""
    seqs = split_sequences(samples)
    n = seqs.shape[1]
    S = np.zeros((max_lag,) + seqs.shape[2:])
    for t in range(1, min(max_lag, n - 1) + 1):
        S[t - 1] = ((seqs[:, t:] - seqs[:, :n - t]) ** 2).sum(axis=(0, 1))
    return S


def ess_from_stats(var_plus, S, m, n, max_lag):
    """BDA3's split ESS per element from var+ (...) and the lag sums S (>= L', ...), m sequences of n samples.
    -> (ess, mcse, truncated, margin), margin = the smallest |rho_{T+1} + rho_{T+2}| of the truncation decisions taken
    (inf where none was), so a caller can tell which components sit on a knife edge."""
    if n - 1 < 3:
        raise ValueError(f'n = {n} samples per sequence: the truncation rule needs rho up to lag 3 (n >= 4)')
    Lp = min(max_lag, n - 1)
    var_plus = np.asarray(var_plus, dtype=np.float64)
    shape = var_plus.shape
    vp = var_plus.reshape(-1)
    S = np.asarray(S, dtype=np.float64)[:Lp].reshape(Lp, -1)
    t = np.arange(1, Lp + 1, dtype=np.float64).reshape(Lp, 1)
    with np.errstate(divide='ignore', invalid='ignore'):
        rho = 1.0 - S / (m * (n - t)) / (2.0 * vp)
    total = rho[0].copy()
    done = np.zeros(vp.shape, dtype=bool)
    margin = np.full(vp.shape, np.inf)
    T = 1
    while T + 2 <= Lp:
        pair = rho[T] + rho[T + 1]  # rho_{T+1} + rho_{T+2}
        active = ~done
        margin[active] = np.minimum(margin[active], np.abs(pair[active]))
        stop = active & (pair < 0)
        done |= stop
        cont = active & ~stop
        total[cont] += pair[cont]
        T += 2
    truncated = ~done
    tau = 1.0 + 2.0 * total
    mn = m * n
    cap = mn * max(1.0, math.log10(mn))
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        ess = np.where(tau > mn / cap, mn / tau, cap)
        const = vp == 0
        bad = ~np.isfinite(vp) | (~const & ~np.isfinite(tau))
        ess = np.where(const, float(mn), np.where(bad, 0.0, ess))
        truncated = truncated & ~const & ~bad
        margin = np.where(const | bad, np.inf, margin)
        mcse = np.where(const, 0.0, np.where(bad, np.inf, np.sqrt(vp / ess)))
    return ess.reshape(shape), mcse.reshape(shape), truncated.reshape(shape), margin.reshape(shape)


def split_ess_np(samples, max_lag):
    """samples (C, N, ...) -> (ess, mcse, truncated, margin) per trailing element"""
    samples = np.asarray(samples, dtype=np.float64)
    C, N = samples.shape[:2]
    return ess_from_stats(var_plus_np(samples), variogram_np(samples, max_lag), 2 * C, N // 2, max_lag)


def split_ess_map_np(samples, max_lag):
    """samples (C, N, 3, D, H, W) -> per voxel (ess min over the components, mcse max, truncated any, margin min)"""
    ess, mcse, tr, margin = split_ess_np(samples, max_lag)
    return ess.min(axis=0), mcse.max(axis=0), tr.any(axis=0), margin.min(axis=0)
