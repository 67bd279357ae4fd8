"""float64 numpy restatement of the split-R-hat estimator, shared by the host and GPU tests."""
import numpy as np


def split_rhat_np(samples):
    """samples (C, N, ...) -> split-R-hat per trailing element.  Half 0: samples 0 .. N//2 - 1, half 1: the last N//2;
    W = mean of the sequence variances, B/n = variance of the sequence means, R = sqrt(((n-1)/n W + B/n) / W);
    1 where W = B = 0, inf where W = 0 < B."""
    samples = np.asarray(samples, dtype=np.float64)
    C, N = samples.shape[:2]
    n = N // 2
    seqs = np.concatenate([samples[:, :n], samples[:, N - n:]], axis=0)  # (2C, n, ...)
    W = seqs.var(axis=1, ddof=1).mean(axis=0)
    B_n = seqs.mean(axis=1).var(axis=0, ddof=1)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.sqrt(((n - 1) / n * W + B_n) / W)
    return np.where(W > 0, r, np.where(B_n == 0, 1.0, np.inf))


def split_rhat_map_np(samples):
    """samples (C, N, 3, D, H, W) -> (D, H, W): the largest R-hat over the three components"""
    return split_rhat_np(samples).max(axis=0)
