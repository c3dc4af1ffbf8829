"""The two halves of the FID (gan/compute_scores.py:180-208): the moments of a
set of codes and the Frechet distance between two Gaussians.

``code_moments`` replaces ``part.mean(axis=0)`` / ``np.cov(part,
rowvar=False)`` (:193-197).  Device tensors go to ``smmd_code_moments`` (the
f32 matrix cores with double folding; the gathered rows are read in place);
CPU tensors, and device tensors under ``SMMD_FID_COV=0`` (the A/B switch), take
a plain float64 torch path with the same formula.

``frechet_distance`` replaces :199-206.  It runs in float64 on the host: the
d x d spectral step is small next to the covariances.
"""
from __future__ import annotations

import os

import torch

from . import _lib


def _use_library(codes):
    return codes.is_cuda and os.environ.get('SMMD_FID_COV', '1') != '0'


def _check_index(index, n_rows):
    if index.dim() != 1 or index.dtype != torch.int64:
        raise ValueError('index must be a 1-D int64 tensor')
    if index.numel():
        lo, hi = torch.aminmax(index)          # one host check per call
        lo, hi = int(lo), int(hi)
        if lo < 0 or hi >= n_rows:
            raise ValueError('index out of range [0, %d): min %d, max %d' % (n_rows, lo, hi))


def code_moments(codes, index=None):
    """(mean [d], cov [d, d]) in float64 on the codes' device of the rows
    ``codes[index]`` (all rows when index is None); cov is normalised by
    n - 1 as np.cov does.  ``index`` may repeat rows (bootstrap); entries
    outside [0, len(codes)) raise ValueError."""
    if codes.dim() != 2 or codes.dtype != torch.float32:
        raise ValueError('codes must be a float32 [n, d] tensor')
    n_rows, dim = codes.shape
    if index is not None:
        index = torch.as_tensor(index)
        _check_index(index, n_rows)
        index = index.to(codes.device)
    n = n_rows if index is None else index.numel()
    if n < 2 or dim < 1:
        raise ValueError('need at least 2 rows and 1 column (got %d x %d)' % (n, dim))
    if not _use_library(codes):
        part = (codes if index is None else codes.index_select(0, index)).to(torch.float64)
        mean = part.mean(0)
        xc = part - mean
        cov = (xc.t() @ xc) / (n - 1)
        return mean, (cov + cov.t()) * 0.5
    codes = codes.contiguous()
    if index is not None:
        index = index.contiguous()
    dev = codes.device
    mean = torch.empty(dim, device=dev, dtype=torch.float64)
    cov = torch.empty(dim, dim, device=dev, dtype=torch.float64)
    L = _lib.lib()
    nbytes = L.smmd_code_moments_workspace_bytes(n, dim)
    ws = _lib.workspace('fid_cov', nbytes, dev)
    with _lib.timed('smmd_code_moments'):
        _lib.check(L.smmd_code_moments(_lib.ptr(codes), n_rows, dim, _lib.ptr(index), n,
                                       _lib.ptr(mean), _lib.ptr(cov), _lib.ptr(ws), ws.numel(),
                                       _lib.stream_handle(dev)), 'smmd_code_moments')
    return mean, cov


def frechet_distance(mean_g, cov_g, mean_r, cov_r):
    """|mu_g - mu_r|^2 + tr cov_g + tr cov_r - 2 tr sqrt(cov_g cov_r), float64
    on the host.  With cov_g = V diag(w) V^T (w clamped at 0) and s = V
    diag(sqrt w) V^T, sqrt(cov_g cov_r) has the eigenvalues of the symmetric
    M = s cov_r s, so the trace term is sum_i sqrt(max(lambda_i(M), 0)): the
    reference's sqrtm trace wherever that is real and finite, and defined on
    singular covariances too (no eps retry)."""
    mg, cg, mr, cr = (torch.as_tensor(t).detach().to('cpu', torch.float64)
                      for t in (mean_g, cov_g, mean_r, cov_r))
    w, V = torch.linalg.eigh((cg + cg.t()) * 0.5)
    s = (V * w.clamp_min(0).sqrt()) @ V.t()
    M = s @ cr @ s
    lam = torch.linalg.eigvalsh((M + M.t()) * 0.5)
    tr_sqrt = lam.clamp_min(0).sqrt().sum()
    diff = mg - mr
    return float(diff.dot(diff) + torch.trace(cg) + torch.trace(cr) - 2.0 * tr_sqrt)


__all__ = ['code_moments', 'frechet_distance']
