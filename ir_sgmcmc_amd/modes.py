"""Posterior principal modes: PCA of the recorded displacement fields by the snapshot method.

Every other posterior summary is per voxel; this one says how the uncertainty at one voxel is tied to the uncertainty at another.
The covariance of the displacement field is (3V)^2, but with n records its rank is at most n - 1, and everything comes from the
n x n Gram matrix of the records.  The records are kept on the device (`modes_state`: a store of cap x 3 x D x H x W float32),
the Gram matrix is maintained as they arrive (`modes_append`: irs_modes_gram_rows, per channel, float64, a fixed summation order)
and at the end the host diagonalises it (`modes_decompose`, float64 numpy) and one pass over the store forms the mean, the mode
fields and the explained-variance map (`modes_project`: irs_modes_project).  include/irsgmcmc.h has the arithmetic, element by
element; DESIGN.md section 6 ("Displacement modes") the definitions.

The operator wrappers live here and not in ops.py; they use its private helpers.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib as L
from .ops import _call, _volume_mask, _workspace


def modes_state(dims, cap, device, mask=None):
    """dims (D,H,W); cap: the most records the store holds, 1 .. IRS_MODES_MAX_RECORDS; mask: bool / uint8 volume of D H W
    elements or None, fixed from here on -> {'store': (cap,3,D,H,W) float32, 'gram': (3,cap,cap) float64 zeros, 'mask': uint8
    or None, 'n': records so far, 'mask_voxels': voxels the mask admits}.  12 V cap bytes of store."""
    dims = tuple(int(d) for d in dims)
    if len(dims) != 3 or min(dims) < 1:
        raise L.IrsError(f'dims must be three extents of at least 1, got {dims!r}')
    cap = int(cap)
    if not 1 <= cap <= L.IRS_MODES_MAX_RECORDS:
        raise L.IrsError(f'cap = {cap} records, 1..{L.IRS_MODES_MAX_RECORDS}')
    if mask is not None:
        mask = _volume_mask(mask.to(device), *dims).contiguous()
    voxels = int(np.prod(dims)) if mask is None else int(mask.count_nonzero().item())
    return {'store': torch.empty((cap, 3, *dims), device=device, dtype=torch.float32),
            'gram': torch.zeros((3, cap, cap), device=device, dtype=torch.float64), 'mask': mask, 'n': 0, 'mask_voxels': voxels,
            'ws': {}}


def _state(state):
    store = state['store']
    if store.dim() != 5 or store.shape[1] != 3:
        raise L.IrsError(f'state["store"] must have shape (cap,3,D,H,W), got {tuple(store.shape)}')
    return store, store.shape[0], tuple(store.shape[2:])


def modes_append(state, displacement):
    """The (C,3,D,H,W) float32 displacements of one step, chains in order, C in 1 .. IRS_MAX_CHAINS: copied into the next C slots
    of the store, then one irs_modes_gram_rows call fills their rows and columns of the Gram matrix.  No host synchronisation."""
    store, cap, dims = _state(state)
    if displacement.dim() != 5 or tuple(displacement.shape[1:]) != (3, *dims):
        raise L.IrsError(f'displacement must have shape (C,3,{dims[0]},{dims[1]},{dims[2]}), got {tuple(displacement.shape)}')
    C, n = displacement.shape[0], state['n']
    if not 1 <= C <= L.IRS_MAX_CHAINS:
        raise L.IrsError(f'displacement of {C} chains, 1..{L.IRS_MAX_CHAINS}')
    if n + C > cap:
        raise L.IrsError(f'{n} records + {C} chains exceed the store\'s cap of {cap}')
    L.dev_ptr(displacement, torch.float32)
    store[n:n + C].copy_(displacement)
    if C not in state['ws']:  # one workspace per number of new records, kept: a recorded step allocates nothing
        state['ws'][C] = _workspace('irs_modes_gram_workspace', *dims, C, device=store.device)
    ws, ws_bytes = state['ws'][C]
    _call('irs_modes_gram_rows', L.dev_ptr(store, torch.float32), cap, n, C, *dims, L.dev_ptr(state['mask'], torch.uint8, allow_none=True),
          L.dev_ptr(state['gram'], torch.float64), L.dev_ptr(ws), ws_bytes)
    state['n'] = n + C


def modes_gram(state):
    """-> the (3,n,n) float64 Gram matrix of the n records so far, on the host (numpy).  Blocking."""
    n = state['n']
    return state['gram'][:, :n, :n].cpu().numpy()


def split_rhat_series(series):
    """scalar split-R-hat (Gelman et al., BDA3 section 11.4) of `series` (C, N): every chain's N values in order, halves of
    N // 2 (the middle one of an odd count goes to neither) -- ops.split_rhat's formula: sqrt(var+ / W), 1 where W = B = 0, inf
    where W = 0 < B"""
    C, N = series.shape
    h = N // 2
    halves = np.concatenate([series[:, :h], series[:, N - h:]], axis=0)  # the 2C sequences
    means = halves.mean(axis=1)
    W = float(np.mean(((halves - means[:, None]) ** 2).sum(axis=1) / (h - 1)))
    B = float(means.var(ddof=1))  # the variance of the sequence means
    if W == 0.0:
        return 1.0 if B == 0.0 else math.inf
    return math.sqrt(((h - 1) / h * W + B) / W)


def modes_decompose(G3, scale, mask_voxels, chain=None, M=8):
    """The host algebra of the snapshot PCA, float64 numpy; usable without a GPU.  G3 (3,n,n): the per-channel Gram matrices;
    scale: three floats, the units of the channels; mask_voxels: |mask|; chain (n,): the chain of every record or None; M: modes
    wanted (at most n - 1 are returned).
    G = sum_c s_c^2 G3[c]; Gc = H G H / (n - 1) with H = I - 11^T / n; eigenpairs of Gc in decreasing order, the eigenvalues
    clamped at 0, every eigenvector with its entry of largest magnitude positive (lowest index on a tie).
    -> {'n', 'eigenvalues' (n-1,), 'var_total', 'explained' (n-1,), 'n90', 'participation', 'std' (n-1,), 'scores' (n,K),
    'coeff' (K,n): the coefficients of the 1-sigma mode fields in record units, 'eigenvectors' (n,K), 'rhat' (K,)}, K = min(M,
    n - 1).  n = 1: no mode (K = 0), var_total 0."""
    G3 = np.asarray(G3, dtype=np.float64)
    if G3.ndim != 3 or G3.shape[0] != 3 or G3.shape[1] != G3.shape[2] or G3.shape[1] < 1:
        raise ValueError(f'G3 must have shape (3, n, n) with n >= 1, got {G3.shape}')
    n = G3.shape[1]
    s = np.asarray(scale, dtype=np.float64).reshape(3)
    G = s[0] * s[0] * G3[0] + s[1] * s[1] * G3[1] + s[2] * s[2] * G3[2]
    K = max(min(int(M), n - 1), 0)
    nan = float('nan')
    if n < 2:
        return {'n': n, 'eigenvalues': np.zeros(0), 'var_total': 0.0, 'explained': np.zeros(0), 'n90': 0, 'participation': nan,
                'std': np.zeros(0), 'scores': np.zeros((n, 0)), 'coeff': np.zeros((0, n)), 'eigenvectors': np.zeros((n, 0)),
                'rhat': np.zeros(0)}
    H = np.eye(n) - np.full((n, n), 1.0 / n)
    Gc = H @ G @ H / (n - 1)
    Gc = 0.5 * (Gc + Gc.T)
    w, U = np.linalg.eigh(Gc)
    order = np.argsort(-w, kind='stable')[:n - 1]  # the centring leaves rank n - 1: the smallest is the null direction
    lam = np.maximum(w[order], 0.0)
    U = U[:, order]
    for m in range(U.shape[1]):
        if U[np.argmax(np.abs(U[:, m])), m] < 0:
            U[:, m] = -U[:, m]
    var_total = float(np.trace(Gc))
    explained = lam / var_total if var_total > 0 else np.zeros_like(lam)
    cum = np.cumsum(explained)
    reached = np.nonzero(cum >= 0.9)[0]
    n90 = int(reached[0]) + 1 if reached.size else len(lam)
    sq = float(np.sum(lam * lam))
    participation = float(np.sum(lam)) ** 2 / sq if sq > 0 else nan
    std = np.sqrt(lam / mask_voxels) if mask_voxels > 0 else np.full_like(lam, nan)
    scores = np.sqrt((n - 1) * lam[:K])[None, :] * U[:, :K]
    coeff = (H @ U[:, :K]).T / math.sqrt(n - 1)
    rhat = np.full(K, nan)
    if chain is not None and K > 0:
        chain = np.asarray(chain).reshape(n)
        ids = np.unique(chain)
        counts = [int(np.sum(chain == c)) for c in ids]
        if len(ids) >= 2 and min(counts) >= 4:
            N = min(counts)
            for m in range(K):
                rhat[m] = split_rhat_series(np.stack([scores[chain == c, m][:N] for c in ids]))
    return {'n': n, 'eigenvalues': lam, 'var_total': var_total, 'explained': explained, 'n90': n90, 'participation': participation,
            'std': std, 'scores': scores, 'coeff': np.ascontiguousarray(coeff), 'eigenvectors': U[:, :K], 'rhat': rhat}


def modes_project(state, coeff, scale):
    """coeff (M,n) float64 (numpy or tensor), M in 1 .. IRS_MODES_MAX, n the records so far; scale: three positive floats ->
    (mean (3,D,H,W), modes (M,3,D,H,W), explained (D,H,W)) float32 on the device, one pass over the store (irs_modes_project)."""
    store, _, dims = _state(state)
    n = state['n']
    coeff = torch.as_tensor(np.array(coeff) if isinstance(coeff, np.ndarray) else coeff)  # (a copy: torch wants it writable)
    if coeff.dim() != 2 or coeff.shape[1] != n or coeff.dtype != torch.float64:
        raise L.IrsError(f'coeff must be float64 of shape (M,{n}), got {coeff.dtype} {tuple(coeff.shape)}')
    M = coeff.shape[0]
    coeff = coeff.to(store.device).contiguous()
    mean = torch.empty((3, *dims), device=store.device, dtype=torch.float32)
    modes = torch.empty((max(M, 0), 3, *dims), device=store.device, dtype=torch.float32)
    explained = torch.empty(dims, device=store.device, dtype=torch.float32)
    sc = (ctypes.c_double * 3)(*(float(s) for s in scale))
    _call('irs_modes_project', L.dev_ptr(store, torch.float32), n, *dims, L.dev_ptr(coeff, torch.float64), M, sc, L.dev_ptr(mean),
          L.dev_ptr(modes) if M > 0 else None, L.dev_ptr(explained))
    return mean, modes, explained
