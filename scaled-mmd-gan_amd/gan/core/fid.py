"""The two halves of the FID (gan/compute_scores.py:180-208): the moments of a
set of codes and the Frechet distance between two Gaussians.

``code_moments`` replaces ``part.mean(axis=0)`` / ``np.cov(part,
rowvar=False)`` (:193-197).  Device tensors go to ``smmd_code_moments`` (the
f32 matrix cores with double folding; the gathered rows are read in place);
CPU tensors, and device tensors under ``SMMD_FID_COV=0`` (the A/B switch), take
a plain float64 torch path with the same formula.

``frechet_distance`` replaces :199-206.  Its spectral step runs in float64 on
the host by default (two ``eigh``); ``spectral='device'`` (or
``SMMD_FID_SQRT=1``) takes the trace of the square root from
``smmd_fid_trace_sqrt`` instead: a shifted Newton-Schulz iteration of f64
matrix-core products on the covariances where ``code_moments`` left them.
"""
from __future__ import annotations

import math
import os
import warnings

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


SQRT_DELTA = 1e-14            # the shift of the device spectral step
SQRT_RESIDUAL_MAX = 1e-6      # a larger residual of either root: the host value
_warned = False


def sqrt_iters(delta):
    """Newton-Schulz iterations of the device spectral step: the smallest
    eigenvalue of the shifted input, delta, grows 1.5x per iteration until its
    root sqrt(delta) is reached, then 12 quadratic ones."""
    return int(math.ceil(math.log(delta ** -0.5) / math.log(1.5))) + 12


def trace_sqrt(cov_g, cov_r):
    """``smmd_fid_trace_sqrt`` on two float64 device covariances (delta =
    SQRT_DELTA and its iteration count): a device tensor {tr sqrt(cov_g cov_r),
    residual of stage 1, residual of stage 3, c3}, enqueued on the current
    stream, nothing read back."""
    for t in (cov_g, cov_r):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float64):
            raise _lib.SmmdError("the device spectral step needs float64 device covariances "
                                 "(got %s on %s)" % (getattr(t, 'dtype', type(t)),
                                                     getattr(t, 'device', 'the host')))
    dim = cov_g.shape[-1]
    if cov_g.shape != (dim, dim) or cov_r.shape != (dim, dim):
        raise ValueError('covariances must be square and of one size')
    cov_g, cov_r = cov_g.contiguous(), cov_r.contiguous()
    dev = cov_g.device
    out4 = torch.empty(4, device=dev, dtype=torch.float64)
    L = _lib.lib()
    ws = _lib.workspace('fid_sqrt', L.smmd_fid_trace_sqrt_workspace_bytes(dim), dev)
    with _lib.timed('smmd_fid_trace_sqrt'):
        _lib.check(L.smmd_fid_trace_sqrt(_lib.ptr(cov_g), _lib.ptr(cov_r), dim, SQRT_DELTA,
                                         sqrt_iters(SQRT_DELTA), _lib.ptr(out4), _lib.ptr(ws),
                                         ws.numel(), _lib.stream_handle(dev)),
                   'smmd_fid_trace_sqrt')
    return out4


def _frechet_device(mean_g, cov_g, mean_r, cov_r):
    """The score with the trace term from ``trace_sqrt``; |mu_g - mu_r|^2 and
    the traces on the device, one small tensor read back.  None (after one
    warning) when a residual says that an iteration did not converge."""
    global _warned
    out4 = trace_sqrt(cov_g, cov_r)
    diff = (torch.as_tensor(mean_g).to(cov_g.device, torch.float64)
            - torch.as_tensor(mean_r).to(cov_g.device, torch.float64))
    head = torch.stack([diff.dot(diff), torch.trace(cov_g), torch.trace(cov_r)])
    d2, tr_g, tr_r, tr_sqrt, res1, res3, _ = torch.cat([head, out4]).tolist()
    if not (res1 <= SQRT_RESIDUAL_MAX and res3 <= SQRT_RESIDUAL_MAX):     # nan included
        if not _warned:
            _warned = True
            warnings.warn('device spectral step: residuals %.3e and %.3e (limit %.1e); the '
                          'host eigen step scores instead' % (res1, res3, SQRT_RESIDUAL_MAX))
        return None
    return d2 + tr_g + tr_r - 2.0 * tr_sqrt


def frechet_distance(mean_g, cov_g, mean_r, cov_r, spectral=None):
    """|mu_g - mu_r|^2 + tr cov_g + tr cov_r - 2 tr sqrt(cov_g cov_r).

    ``spectral='host'`` (the default; None reads ``SMMD_FID_SQRT``, '1' =
    device): float64 on the host.  With cov_g = V diag(w) V^T (w clamped at 0)
    and s = V diag(sqrt w) V^T, sqrt(cov_g cov_r) has the eigenvalues of the
    symmetric M = s cov_r s, so the trace term is sum_i sqrt(max(lambda_i(M),
    0)): the reference's sqrtm trace wherever that is real and finite, and
    defined on singular covariances too (no eps retry).

    ``spectral='device'``: the trace term by the shifted Newton-Schulz
    iteration on the f64 matrix cores (``smmd_fid_trace_sqrt``); float64 device
    covariances or SmmdError.  The shift costs up to about 1e-6 of the traces
    on rank-deficient covariances, which is why it is opt-in."""
    if spectral is None:
        spectral = 'device' if os.environ.get('SMMD_FID_SQRT') == '1' else 'host'
    if spectral not in ('host', 'device'):
        raise ValueError("spectral must be 'host' or 'device' (got %r)" % (spectral,))
    if spectral == 'device':
        score = _frechet_device(mean_g, cov_g, mean_r, cov_r)
        if score is not None:
            return score
    mg, cg, mr, cr = (torch.as_tensor(t).detach().to('cpu', torch.float64)
                      for t in (mean_g, cov_g, mean_r, cov_r))
    w, V = torch.linalg.eigh((cg + cg.t()) * 0.5)
    s = (V * w.clamp_min(0).sqrt()) @ V.t()
    M = s @ cr @ s
    lam = torch.linalg.eigvalsh((M + M.t()) * 0.5)
    tr_sqrt = lam.clamp_min(0).sqrt().sum()
    diff = mg - mr
    return float(diff.dot(diff) + torch.trace(cg) + torch.trace(cr) - 2.0 * tr_sqrt)


__all__ = ['code_moments', 'frechet_distance', 'trace_sqrt', 'sqrt_iters']
